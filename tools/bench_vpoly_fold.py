"""Times one prover round of the R1CS claim  c0 e a b - e c  -- the fold of every distinct table at the challenge, then the next round's
message -- on the GPU in three ways (DESIGN_APPENDIX.md A.13; raw output: profiles/vpoly_fold/).

For each table shape and both orders, in one child process per shape (each under its own time limit) and alternating per repetition:
  (a)  the fused call: sr_vpoly_round_fold_evals_dev;
  (b1) a fold per distinct table (sr_mle_fix_variables_dev, n_fixed = 1), then sr_vpoly_round_evals_dev on the folded tables;
  (b2) the hand composition: sr_mle_round_fold_evals_dev(e, a, b), a fold of c, sr_mle_round_evals_dev(e', c'), the second message
       extrapolated to t = 3 (q(3) = q(0) + 3 (q(2) - q(1))), the first scaled by c0, and the difference;
  (c)  add_dev on the two halves of one table: the streaming rate of the box in this run.
Device events sit around every timed piece; every shape is warmed up first and the three results are compared bit for bit in the same
run.  `bytes` is the table traffic of the piece over four tables of n: 1.5 n per table for (a), plus 0.5 n per table for every launch
of remaining points; 2 n per table for (b1); 1.5 n for e, a, b, 1.5 n for c and 0.5 n each for e', c' in (b2).  The ratios a / b1 and
a / b2 are taken per repetition; the spread of (b1) is the margin.  Prints one JSON line per (shape, order).

    python tools/bench_vpoly_fold.py [--reps 10] [--small] [--out FILE] [--timeout 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TABLES = [("goldilocks", 10, 20), ("goldilocks", 16, 14), ("babybear", 16, 14), ("stark", 12, 12), ("goldilocks24", 0, 24)]
SMALL = [("goldilocks", 10, 14), ("goldilocks", 16, 8), ("babybear", 16, 8), ("stark", 12, 8), ("goldilocks24", 0, 18)]
ORDERS = (("leading", 0), ("trailing", 1))
R1CS = [[0, 1, 2], [0, 3]]


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def run_shape(name, k, nv, reps):
    import torch

    from stark_rings_amd import CyclotomicRing

    assert torch.cuda.is_available(), "bench_vpoly_fold needs a GPU"
    ring = CyclotomicRing(name, k, device=0)
    w = ring.words_per_elem
    eb, n = w * 8, 1 << nv
    new = lambda elems: torch.empty(elems * w, dtype=torch.int64, device="cuda")  # noqa: E731
    tables = []
    for j in range(4):
        t = new(n)
        ring.fill_uniform_dev(t, 0x5D00 + j, 0)
        tables.append(t)
    r, coeffs = new(1), new(2)
    ring.fill_uniform_dev(r, 0x5DFF, 0)
    ring.fill_uniform_dev(coeffs, 0x5DFE, 0)
    ring.eq_table_dev(coeffs[w:], None)   # one()
    ring.neg_dev(coeffs[w:])              # c1 = -one()
    c0 = coeffs[:w].clone()
    half = (n // 2) * eb
    out_t = {key: [new(n // 2) for _ in range(4)] for key in ("a", "b1", "b2")}
    for order_name, order in ORDERS:
        work_elems, launches = ring.vpoly_round_fold_plan(nv, 4, 2, 3, order)
        work = new(max(work_elems, 1))
        v_elems, v_launches = ring.vpoly_round_plan(nv - 1, 4, 2, 3, order)
        v_work = new(max(v_elems, 1))
        f_elems, f_launches = ring.mle_round_fold_plan(nv, 3, order)
        f_work = new(max(f_elems, 1))
        m_elems, m_launches = ring.mle_round_plan(nv - 1, 2, order)
        m_work = new(max(m_elems, 1))
        out = {key: new(4) for key in ("a", "b1", "b2")}
        q = new(4)

        def run_a():
            ring.vpoly_round_fold_evals_dev(out["a"], out_t["a"], tables, R1CS, coeffs, nv, r, order, work if work_elems else None)

        def run_b1():
            for j in range(4):
                ring.mle_fix_variables_dev(out_t["b1"][j], tables[j], nv, r, order, None)
            ring.vpoly_round_evals_dev(out["b1"], out_t["b1"], R1CS, coeffs, nv - 1, order, v_work if v_elems else None)

        dq = new(1)

        def run_b2():
            o, t = out["b2"], out_t["b2"]
            ring.mle_round_fold_evals_dev(o, t[:3], tables[:3], nv, r, order, f_work if f_elems else None)
            ring.mle_fix_variables_dev(t[3], tables[3], nv, r, order, None)
            ring.mle_round_evals_dev(q[:3 * w], [t[0], t[3]], nv - 1, order, m_work if m_elems else None)
            q3 = q[3 * w:]
            q3.copy_(q[2 * w:3 * w])
            ring.sub_dev(q3, q[w:2 * w])             # dq = q(2) - q(1)
            dq.copy_(q3)
            ring.add_dev(q3, dq)
            ring.add_dev(q3, dq)                # 3 dq
            ring.add_dev(q3, q[:w])                  # q(3) = q(0) + 3 (q(2) - q(1))
            ring.mul_elem_dev(o, c0)                 # c0 p(t), t = 0 .. 3
            ring.sub_dev(o, q)                       # - q(t)

        pieces = {"a_fused": run_a, "b1_folds_then_vpoly": run_b1, "b2_hand_composition": run_b2,
                  "c_add": lambda: ring.add_dev(out_t["a"][3], out_t["b1"][3])}
        rest_launches = launches - 1 - (1 if work_elems else 0)
        nbytes = {"a_fused": 4 * (3 + rest_launches) * half, "b1_folds_then_vpoly": 4 * (3 + v_launches - (1 if v_elems else 0)) * half,
                  "b2_hand_composition": (3 * 3 + 3 + 2) * half, "c_add": 3 * half}
        for f in (run_a, run_b1, run_b2):
            f()
            f()
        torch.cuda.synchronize()
        same = {key: bool(torch.equal(out["a"], out[key])) and all(bool(torch.equal(x, y)) for x, y in zip(out_t["a"], out_t[key]))
                for key in ("b1", "b2")}
        ms = {key: [] for key in pieces}
        for _ in range(reps):
            for key, f in pieces.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                ms[key].append(a.elapsed_time(b))
        res = {"ring": name, "log2_degree": k, "num_vars": nv, "structure": "R1CS", "order": order_name, "table_bytes": n * eb, "reps": reps,
               "launches": launches, "launches_b1": 4 + v_launches, "launches_b2": f_launches + 1 + m_launches + 7, "work_elems": work_elems,
               "fused_equals_b1": same["b1"], "fused_equals_b2": same["b2"]}
        for key in pieces:
            med = statistics.median(ms[key])
            res[key] = {"ms_median": round(med, 4), "ms_min": round(min(ms[key]), 4), "ms_max": round(max(ms[key]), 4),
                        "bytes": nbytes[key], "tb_per_s": round(nbytes[key] / (med * 1e-3) / 1e12, 3)}
        res["a_over_b1"] = spread([x / y for x, y in zip(ms["a_fused"], ms["b1_folds_then_vpoly"])])
        res["a_over_b2"] = spread([x / y for x, y in zip(ms["a_fused"], ms["b2_hand_composition"])])
        med_b1 = statistics.median(ms["b1_folds_then_vpoly"])
        res["b1_spread"] = spread([x / med_b1 for x in ms["b1_folds_then_vpoly"]])
        print(json.dumps(res), flush=True)
    ring.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="tables 2^6 times smaller (a quick check of the tool itself)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=240, help="seconds one shape's child process may take")
    ap.add_argument("--shape", default=None, help="(internal) ring,log2_degree,num_vars: run this shape in this process")
    args = ap.parse_args()
    if args.shape:
        name, k, nv = args.shape.split(",")
        run_shape(name, int(k), int(nv), args.reps)
        return 0
    lines = []
    for name, k, nv in (SMALL if args.small else TABLES):
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--shape", "%s,%d,%d" % (name, k, nv)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("bench_vpoly_fold: %s 2^%d x 2^%d ran past %d s; stopping" % (name, k, nv, args.timeout), file=sys.stderr)
            return 124
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:  # a failed step ends the run: nothing more is started on the device
            sys.stderr.write(r.stderr)
            return r.returncode
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
