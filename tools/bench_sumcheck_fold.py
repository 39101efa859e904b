"""Times one prover round -- the fold at the challenge, then the next round's message -- on the GPU in two ways (DESIGN_APPENDIX.md
A.10; raw output: profiles/sumcheck_fold/).

For each table shape, d = 2, 3 tables and both orders, in one child process per shape (each under its own time limit) and alternating
per repetition:
  (a) the fused call: sr_mle_round_fold_evals_dev;
  (b) the two calls it merges: sr_mle_fix_variables_dev (n_fixed = 1) per table, then sr_mle_round_evals_dev on the folded tables;
  (c) add_dev on the two halves of one table: the streaming rate of the box in this run.
Device events sit around every timed piece; every shape is warmed up first.  `bytes` is the table traffic of the piece: 1.5 n per table
for (a), 2 n for (b) (the fold reads n and writes n / 2, the message reads the n / 2); tb_per_s is that over the median time.
Prints one JSON line per (shape, d, order).

    python tools/bench_sumcheck_fold.py [--reps 10] [--small] [--out FILE] [--timeout 240]
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


def run_shape(name, k, nv, reps):
    import torch

    from stark_rings_amd import CyclotomicRing

    assert torch.cuda.is_available(), "bench_sumcheck_fold needs a GPU"
    ring = CyclotomicRing(name, k, device=0)
    w = ring.words_per_elem
    eb, n = w * 8, 1 << nv
    tables = []
    for j in range(3):
        t = torch.empty(n * w, dtype=torch.int64, device="cuda")
        ring.fill_uniform_dev(t, 0x5C00 + j, 0)
        tables.append(t)
    r = torch.empty(w, dtype=torch.int64, device="cuda")
    ring.fill_uniform_dev(r, 0x5CFF, 0)
    half = (n // 2) * eb
    out_a_t = [torch.empty((n // 2) * w, dtype=torch.int64, device="cuda") for _ in range(3)]
    out_b_t = [torch.empty((n // 2) * w, dtype=torch.int64, device="cuda") for _ in range(3)]
    for d in (2, 3):
        for order_name, order in ORDERS:
            work_elems, launches = ring.mle_round_fold_plan(nv, d, order)
            work = torch.empty(max(work_elems, 1) * w, dtype=torch.int64, device="cuda")
            rwork_elems, rlaunches = ring.mle_round_plan(nv - 1, d, order)
            rwork = torch.empty(max(rwork_elems, 1) * w, dtype=torch.int64, device="cuda")
            out_a = torch.empty((d + 1) * w, dtype=torch.int64, device="cuda")
            out_b = torch.empty((d + 1) * w, dtype=torch.int64, device="cuda")

            def run_a():
                ring.mle_round_fold_evals_dev(out_a, out_a_t[:d], tables[:d], nv, r, order, work if work_elems else None)

            def run_b():
                for j in range(d):
                    ring.mle_fix_variables_dev(out_b_t[j], tables[j], nv, r, order, None)
                ring.mle_round_evals_dev(out_b, out_b_t[:d], nv - 1, order, rwork if rwork_elems else None)

            def run_c():
                ring.add_dev(out_a_t[2], out_b_t[2])

            pieces = {"a_fused": run_a, "b_two_calls": run_b, "c_add": run_c}
            nbytes = {"a_fused": d * 3 * half, "b_two_calls": d * 4 * half, "c_add": 3 * half}
            for f in (run_a, run_b):
                f()
                f()
            torch.cuda.synchronize()
            same = bool(torch.equal(out_a, out_b)) and all(bool(torch.equal(x, y)) for x, y in zip(out_a_t[:d], out_b_t[:d]))
            ms = {key: [] for key in pieces}
            for _ in range(reps):
                for key, f in pieces.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    f()
                    b.record()
                    b.synchronize()
                    ms[key].append(a.elapsed_time(b))
            res = {"ring": name, "log2_degree": k, "num_vars": nv, "tables": d, "order": order_name, "table_bytes": n * eb, "reps": reps,
                   "launches": launches, "launches_two_calls": d + rlaunches, "work_elems": work_elems, "fused_equals_two_calls": same}
            for key in pieces:
                med = statistics.median(ms[key])
                res[key] = {"ms_median": round(med, 4), "ms_min": round(min(ms[key]), 4), "ms_max": round(max(ms[key]), 4),
                            "bytes": nbytes[key], "tb_per_s": round(nbytes[key] / (med * 1e-3) / 1e12, 3)}
            res["fused_over_two_calls_time"] = round(res["a_fused"]["ms_median"] / res["b_two_calls"]["ms_median"], 4)
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
            print("bench_sumcheck_fold: %s 2^%d x 2^%d ran past %d s; stopping" % (name, k, nv, args.timeout), file=sys.stderr)
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
