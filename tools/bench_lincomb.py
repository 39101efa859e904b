"""Times linear combinations of tables on the GPU (DESIGN_APPENDIX.md A.17; raw output: profiles/lincomb/).

For each table shape, in one child process per shape (each under its own time limit), and for each (K, M) point -- (3, 2): the
permutation leaves, whose rows each leave out one table; (4, 1), (8, 1), (16, 1): fingerprints and folds -- alternating per repetition:
  (a)  the new call, sr_lincomb_dev: one pass (several launches where the plan splits the outputs);
  (b)  the composition a caller had before it, per output: a device copy of the first used table, sr_mul_elem_batch_dev by its
       coefficient, sr_mul_elem_add_batch_dev per further table, sr_add_scalar_batch_dev for the constant (a base-field scalar times
       one(), prepared outside the timed piece);
  (d)  add_dev on two tables: the streaming rate of the box in this run.
Device events sit around every timed piece; every variant is warmed up first, and before any time counts (a) is compared bit for bit
with (b).  `elems` is the traffic model of the piece in ring elements: (K + M) n for (a) -- per output the tables its mask uses, per
launch -- M (3 K + 3) n for (b) with K the tables a row uses, 3 n for (d).  The ratio (a)/(b) is taken per repetition; the spread of
(b) is the margin.  Prints one JSON line per shape and point.

    python tools/bench_lincomb.py [--reps 10] [--small] [--out FILE] [--timeout 300]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (ring, log2 D, log2 n).  The shapes of A.14 are 2^10 x 2^20, 2^16 x 2^14 (Goldilocks, BabyBear), 2^12 x 2^12 (Stark) and 24 x 2^24;
# nineteen tables of 8 GiB do not fit beside the other users of a shared device, so the one-limb shapes are halved twice (2 GiB per
# table) and goldilocks24 once (1.5 GiB); Stark is A.14's (512 MiB).
TABLES = [("goldilocks", 10, 18), ("goldilocks", 16, 12), ("babybear", 16, 12), ("stark", 12, 12), ("goldilocks24", 0, 23)]
SMALL = [("goldilocks", 10, 12), ("goldilocks", 16, 6), ("babybear", 16, 6), ("stark", 12, 6), ("goldilocks24", 0, 17)]
POINTS = [(3, 2, [0b1011, 0b1101]), (4, 1, [0b11111]), (8, 1, [0x1FF]), (16, 1, [0x1FFFF])]


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def run_shape(name, k, nv, reps):
    import numpy as np
    import torch

    from stark_rings_amd import CyclotomicRing, lincomb_dev, lincomb_plan

    assert torch.cuda.is_available(), "bench_lincomb needs a GPU"
    ring = CyclotomicRing(name, k, device=0)
    w = ring.words_per_elem
    eb, n = w * 8, 1 << nv
    new = lambda elems: torch.empty(elems * w, dtype=torch.int64, device="cuda")  # noqa: E731
    kmax = max(p[0] for p in POINTS)
    tables = [new(n) for _ in range(kmax)]
    for j, t in enumerate(tables):
        ring.fill_uniform_dev(t, 0xA800 + j, 0)
    scalar = tables[0][:ring.limbs].cpu().numpy().view(np.uint64).copy()   # one canonical base-field coefficient
    const = torch.zeros(w, dtype=torch.int64, device="cuda")
    ring.add_scalar_dev(const, scalar, True)
    outs_a, outs_b, scratch = [new(n), new(n)], [new(n), new(n)], new(n)
    scratch.zero_()
    for K, M, uses in POINTS:
        coef = new(M * (K + 1))
        ring.fill_uniform_dev(coef, 0xA900 + K, 0)
        for m in range(M):
            coef[(m * (K + 1) + K) * w:(m * (K + 1) + K + 1) * w] = const
        used = [[j for j in range(K) if uses[m] >> j & 1] for m in range(M)]

        def run_a():
            lincomb_dev(ring, outs_a[:M], tables[:K], coef, uses, n)

        def run_b():
            for m in range(M):
                o, row = outs_b[m], coef[m * (K + 1) * w:(m + 1) * (K + 1) * w]
                first = used[m][0]
                o.copy_(tables[first])
                ring.mul_elem_dev(o, row[first * w:(first + 1) * w])
                for j in used[m][1:]:
                    ring.mul_elem_add_dev(o, tables[j], row[j * w:(j + 1) * w])
                ring.add_scalar_dev(o, scalar, True)

        def run_d():
            ring.add_dev(scratch, tables[0])

        pieces = {"a_lincomb": run_a, "b_composition": run_b, "d_add": run_d}
        launches, per = lincomb_plan(ring, K, M)
        elems = {"a_lincomb": sum(len({j for m in range(m0, min(m0 + per, M)) for j in used[m]}) + min(per, M - m0) for m0 in range(0, M, per)) * n,
                 "b_composition": sum(3 * len(u) + 3 for u in used) * n, "d_add": 3 * n}
        for f in (run_a, run_b):
            f()
            f()
        torch.cuda.synchronize()
        same = all(bool(torch.equal(outs_a[m], outs_b[m])) for m in range(M))
        assert same, "lincomb and the composition differ at %s K=%d M=%d" % (name, K, M)   # no time counts unless the variants agree
        run_d()
        ms = {key: [] for key in pieces}
        for _ in range(reps):
            for key, f in pieces.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                ms[key].append(a.elapsed_time(b))
        res = {"ring": name, "log2_degree": k, "log2_n": nv, "n_tables": K, "n_outputs": M, "table_bytes": n * eb, "reps": reps,
               "launches": launches, "outputs_per_launch": per, "a_equals_b": same,
               "model_a_over_b": round(elems["a_lincomb"] / elems["b_composition"], 4)}
        for key in pieces:
            med = statistics.median(ms[key])
            res[key] = {"ms_median": round(med, 4), "ms_min": round(min(ms[key]), 4), "ms_max": round(max(ms[key]), 4), "elems": elems[key],
                        "tb_per_s": round(elems[key] * eb / (med * 1e-3) / 1e12, 3)}
        res["a_over_b"] = spread([x / y for x, y in zip(ms["a_lincomb"], ms["b_composition"])])
        res["b_spread"] = round((max(ms["b_composition"]) - min(ms["b_composition"])) / statistics.median(ms["b_composition"]), 4)
        print(json.dumps(res), flush=True)
    ring.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="tables 2^6 times smaller (a quick check of the tool itself)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=300, help="seconds one shape's child process may take")
    ap.add_argument("--shape", default=None, help="(internal) ring,log2_degree,log2_n: run this shape in this process")
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
            print("bench_lincomb: %s 2^%d x 2^%d ran past %d s; stopping" % (name, k, nv, args.timeout), file=sys.stderr)
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
