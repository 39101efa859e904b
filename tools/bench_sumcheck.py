"""Times the sum-check round message on the GPU (DESIGN_APPENDIX.md, "Sum-check rounds"; raw output: profiles/sumcheck/).

For each table shape and d = 2, 3 tables, in one child process per shape (each under its own time limit) and alternating per
repetition:
  (a) the fused call: sr_mle_round_evals_dev, leading order, all d + 1 points;
  (b) the same message composed from the entry points that existed before it: for each of the d + 1 points, d one-variable folds
      (sr_mle_fix_variables_dev with the point t * one) into temporaries, d - 1 sr_pointwise_mul_batch_dev passes, one sr_sum_batch_dev;
  (c) add_dev on the two halves of one table: the streaming rate of the box in this run.
Device events sit around every timed piece; every shape is warmed up first.  `floor_bytes` is one read of each table, the least the
message can cost; tb_per_s of (a) is floor_bytes over its time.  Prints one JSON line per (shape, d).

    python tools/bench_sumcheck.py [--reps 10] [--small] [--out FILE] [--timeout 240]
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
LEADING = 0


def run_shape(name, k, nv, reps):
    import torch

    from stark_rings_amd import CyclotomicRing

    assert torch.cuda.is_available(), "bench_sumcheck needs a GPU"
    ring = CyclotomicRing(name, k, device=0)
    w = ring.words_per_elem
    eb, n = w * 8, 1 << nv
    tables = []
    for j in range(3):
        t = torch.empty(n * w, dtype=torch.int64, device="cuda")
        ring.fill_uniform_dev(t, 0x5C00 + j, 0)
        tables.append(t)
    one = torch.empty(w, dtype=torch.int64, device="cuda")
    ring.eq_table_dev(one, None)
    points = [torch.zeros(w, dtype=torch.int64, device="cuda")]
    for t in range(1, 4):
        points.append(ring.add_dev(points[-1].clone(), one))
    tmp = [torch.empty((n // 2) * w, dtype=torch.int64, device="cuda") for _ in range(3)]
    lo, hi = tmp[0], tmp[1]
    results = []
    for d in (2, 3):
        work_elems, launches = ring.mle_round_plan(nv, d, LEADING)
        work = torch.empty(max(work_elems, 1) * w, dtype=torch.int64, device="cuda")
        out_a = torch.empty((d + 1) * w, dtype=torch.int64, device="cuda")
        out_b = torch.empty((d + 1) * w, dtype=torch.int64, device="cuda")

        def run_a():
            ring.mle_round_evals_dev(out_a, tables[:d], nv, LEADING, work if work_elems else None)

        def run_b():
            for t in range(d + 1):
                for j in range(d):
                    ring.mle_fix_variables_dev(tmp[j], tables[j], nv, points[t], LEADING, None)
                for j in range(1, d):
                    ring.ntt_mul_dev(tmp[0], tmp[j])
                ring.sum_dev(out_b[t * w:(t + 1) * w], tmp[0])

        def run_c():
            ring.add_dev(lo, hi)

        pieces = {"a_fused": run_a, "b_composed": run_b, "c_add": run_c}
        half = (n // 2) * eb
        # (b): per point d folds (read n, write n / 2), d - 1 products (read 2, write 1 half-tables), a sum (read one half-table)
        nbytes = {"a_fused": d * n * eb, "b_composed": (d + 1) * (d * 3 * half + (d - 1) * 3 * half + half), "c_add": 3 * half}
        for f in (run_a, run_b):
            f()
            f()
        torch.cuda.synchronize()
        same = bool(torch.equal(out_a, out_b))
        ms = {key: [] for key in pieces}
        for _ in range(reps):
            for key, f in pieces.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                ms[key].append(a.elapsed_time(b))
        res = {"ring": name, "log2_degree": k, "num_vars": nv, "tables": d, "table_bytes": n * eb, "floor_bytes": d * n * eb, "reps": reps,
               "launches": launches, "work_elems": work_elems, "fused_equals_composed": same}
        for key in pieces:
            med = statistics.median(ms[key])
            res[key] = {"ms_median": round(med, 4), "ms_min": round(min(ms[key]), 4), "ms_max": round(max(ms[key]), 4),
                        "bytes": nbytes[key], "tb_per_s": round(nbytes[key] / (med * 1e-3) / 1e12, 3)}
        res["fused_over_composed_time"] = round(res["a_fused"]["ms_median"] / res["b_composed"]["ms_median"], 4)
        res["fused_share_of_add_rate"] = round(res["a_fused"]["tb_per_s"] / res["c_add"]["tb_per_s"], 3)
        print(json.dumps(res), flush=True)
        results.append(res)
    ring.close()
    return results


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
            print("bench_sumcheck: %s 2^%d x 2^%d ran past %d s; stopping" % (name, k, nv, args.timeout), file=sys.stderr)
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
