"""Times the dense multilinear-extension folds on the GPU (DESIGN_APPENDIX.md, "Multilinear folds"; raw output: profiles/mle/).

For each table, in one process and alternating per repetition:
  (a) evaluate (all num_vars variables, leading order) by the plan sr_mle_plan chooses;
  (b) evaluate as num_vars one-variable calls of the same kernel (two ping-pong buffers);
  (c) one trailing-order round built from the entry points that existed before the fold kernels: copy, sub, mul_elem, add
      (5 n element transfers for a table of n), against (d) the same round as ONE in-place one-variable trailing fold (1.5 n);
  (e) add_dev on the two halves of the same table: the streaming rate of the box in this run.
Device events sit around every timed piece; every shape is warmed up first.  Bytes are the algorithmic counts, computed here from the
shapes.  Prints one JSON line per table.

    python tools/bench_mle.py [--reps 20] [--small] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TABLES = [("goldilocks", 10, 20), ("goldilocks", 16, 14), ("babybear", 16, 14), ("stark", 12, 12), ("goldilocks24", 0, 24)]
SMALL = [("goldilocks", 10, 14), ("goldilocks", 16, 8), ("babybear", 16, 8), ("stark", 12, 8), ("goldilocks24", 0, 18)]
LEADING, TRAILING = 0, 1


def plan_widths(ring, nv):
    """the variables per launch of the plan for a full evaluation (greedy, widest first), from sr_mle_plan alone"""
    jmax = 3 if ring.mle_plan(3, 3, LEADING)[1] == 1 else 2
    js, left = [], nv
    while left:
        js.append(min(jmax, left))
        left -= js[-1]
    assert len(js) == ring.mle_plan(nv, nv, LEADING)[1]
    return js


def fold_bytes(elem_bytes, nv, widths):
    """bytes one fold moves: every launch reads its table and writes the folded one (the point is negligible)"""
    total, m = 0, nv
    for j in widths:
        total += elem_bytes * ((1 << m) + (1 << (m - j)))
        m -= j
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="tables 2^6 times smaller (a quick check of the tool itself)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from stark_rings_amd import CyclotomicRing

    assert torch.cuda.is_available(), "bench_mle needs a GPU"
    results = []
    for name, k, nv in (SMALL if args.small else TABLES):
        ring = CyclotomicRing(name, k, device=0)
        w = ring.words_per_elem
        eb = w * 8
        n = 1 << nv
        table = torch.empty(n * w, dtype=torch.int64, device="cuda")
        ring.fill_uniform_dev(table, 0xBE9C, 0)
        point = torch.empty(nv * w, dtype=torch.int64, device="cuda")
        ring.fill_uniform_dev(point, 0xBE9D, 0)
        widths = plan_widths(ring, nv)
        work_elems = ring.mle_plan(nv, nv, LEADING)[0]
        work = torch.empty(max(work_elems, 1) * w, dtype=torch.int64, device="cuda")
        out_a = torch.empty(w, dtype=torch.int64, device="cuda")
        out_b = torch.empty(w, dtype=torch.int64, device="cuda")
        ping = torch.empty((n // 2) * w, dtype=torch.int64, device="cuda")
        pong = torch.empty(max(n // 4, 1) * w, dtype=torch.int64, device="cuda")
        tmp = torch.empty((n // 2) * w, dtype=torch.int64, device="cuda")
        lo, hi = table[:(n // 2) * w], table[(n // 2) * w:]
        r_last = point[(nv - 1) * w:]

        def run_a():
            ring.mle_fix_variables_dev(out_a, table, nv, point, LEADING, work)

        def run_b():
            src = table
            for i in range(nv):
                m = nv - i
                dst = out_b if i == nv - 1 else (ping if i % 2 == 0 else pong)[:(w << (m - 1))]
                ring.mle_fix_variables_dev(dst, src, m, point[i * w:(i + 1) * w], LEADING, None)
                src = dst

        def run_c():   # lo += r * (hi - lo) from copy, sub, mul_elem, add
            tmp.copy_(hi)
            ring.sub_dev(tmp, lo)
            ring.mul_elem_dev(tmp, r_last)
            ring.add_dev(lo, tmp)

        def run_d():   # the same round as one in-place trailing fold
            ring.mle_fix_variables_dev(lo, table, nv, r_last, TRAILING, None)

        def run_e():
            ring.add_dev(lo, hi)

        pieces = {"a_plan": run_a, "b_one_var": run_b, "c_old_round": run_c, "d_new_round": run_d, "e_add": run_e}
        nbytes = {"a_plan": fold_bytes(eb, nv, widths), "b_one_var": fold_bytes(eb, nv, [1] * nv), "c_old_round": 5 * n * eb,
                  "d_new_round": 3 * n * eb // 2, "e_add": 3 * (n // 2) * eb}
        for f in pieces.values():   # warm-up of every shape
            f()
            f()
        torch.cuda.synchronize()
        same = bool(torch.equal(out_a, out_b))   # before (c) / (d) / (e) change the table: the two plans agree bit for bit
        ms = {key: [] for key in pieces}
        for _ in range(args.reps):
            for key, f in pieces.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                ms[key].append(a.elapsed_time(b))
        res = {"ring": name, "log2_degree": k, "num_vars": nv, "table_bytes": n * eb, "plan_widths": widths, "reps": args.reps,
               "plan_equals_one_var": same}
        for key in pieces:
            med = statistics.median(ms[key])
            res[key] = {"ms_median": round(med, 4), "ms_min": round(min(ms[key]), 4), "ms_max": round(max(ms[key]), 4),
                        "bytes": nbytes[key], "tb_per_s": round(nbytes[key] / (med * 1e-3) / 1e12, 3)}
        res["plan_over_one_var_time"] = round(res["a_plan"]["ms_median"] / res["b_one_var"]["ms_median"], 3)
        res["one_var_spread"] = round((res["b_one_var"]["ms_max"] - res["b_one_var"]["ms_min"]) / res["b_one_var"]["ms_median"], 3)
        res["old_over_new_round_time"] = round(res["c_old_round"]["ms_median"] / res["d_new_round"]["ms_median"], 2)
        res["one_var_share_of_add_rate"] = round(res["d_new_round"]["tb_per_s"] / res["e_add"]["tb_per_s"], 3)
        print(json.dumps(res), flush=True)
        results.append(res)
        ring.close()
        del table, ping, pong, tmp, work
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for res in results:
                f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
