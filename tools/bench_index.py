"""Times one witness column of permutation leaves two ways on the GPU (DESIGN_APPENDIX.md A.19; raw output: profiles/index_columns/).

For each shape, in one child process per shape (each under its own time limit), alternating per repetition:
  (a)  permutation_leaves_indexed: f as a table, id as a progression, sigma as one u64 per row (sr_lincomb_index_dev, K = 1, J = 2,
       M = 2);
  (b)  permutation_leaves over id and sigma as tables of ring elements (sr_lincomb_dev, K = 3, M = 2), the tables made once by
       from_u64_dev outside the timed piece.  Its kernels are those of csrc/lincomb.hpp, which this library has unchanged.
Device events sit around every timed piece; every variant is warmed up first, and before any time counts the outputs of (a) and (b)
are compared bit for bit.  `elems` is the traffic model of the piece in ring elements, per launch the tables its outputs use plus its
outputs; the 8 bytes per row of sigma are counted in `index_bytes`.  The ratio (a)/(b) is taken per repetition; the spread of (b),
(max - min) / median, is the margin.  Prints one JSON line per shape.

    python tools/bench_index.py [--reps 10] [--small] [--out FILE] [--timeout 300]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (ring, log2 D, log2 n): five tables of n elements live at once (f, id, sigma, two outputs per variant share nothing)
TABLES = [("goldilocks", 16, 12), ("babybear", 16, 12), ("stark", 12, 12), ("goldilocks24", 0, 23)]
SMALL = [("goldilocks", 16, 6), ("babybear", 16, 6), ("stark", 12, 6), ("goldilocks24", 0, 17)]


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def run_shape(name, k, nv, reps):
    import torch

    from stark_rings_amd import (CyclotomicRing, IndexColumn, from_u64_dev, lincomb_index_plan, lincomb_plan, permutation_leaves,
                                 permutation_leaves_indexed)

    assert torch.cuda.is_available(), "bench_index needs a GPU"
    ring = CyclotomicRing(name, k, device=0)
    w = ring.words_per_elem
    eb, n = w * 8, 1 << nv
    new = lambda elems: torch.empty(elems * w, dtype=torch.int64, device="cuda")  # noqa: E731
    f, beta, gamma = new(n), new(1), new(1)
    for j, t in enumerate((f, beta, gamma)):
        ring.fill_uniform_dev(t, 0xAB00 + j, 0)
    sigma = torch.randperm(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)).to(torch.int64) + n
    ident_t = from_u64_dev(ring, IndexColumn(start=n), n, like=f)
    sigma_t = from_u64_dev(ring, sigma, n)
    out_a, out_b = [new(n), new(n)], [new(n), new(n)]

    def run_a():
        permutation_leaves_indexed(ring, f, sigma, beta, gamma, id_start=n, num=out_a[0], den=out_a[1])

    def run_b():
        permutation_leaves(ring, f, ident_t, sigma_t, beta, gamma, num=out_b[0], den=out_b[1])

    pieces = {"a_indexed": run_a, "b_tables": run_b}
    la, pa = lincomb_index_plan(ring, 1, 2, 2)
    lb, pb = lincomb_plan(ring, 3, 2)
    # a launch of both outputs reads each table once; a launch of one output reads f and (b only) the one further table it uses
    elems = {"a_indexed": (1 + 2) * n if la == 1 else 2 * (1 + 1) * n, "b_tables": (3 + 2) * n if lb == 1 else 2 * (2 + 1) * n}
    for fn in (run_a, run_b):
        fn()
        fn()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(x, y)) for x, y in zip(out_a, out_b))
    assert same, "the indexed leaves and the leaves over tables differ at %s" % name   # no time counts unless the variants agree
    ms = {key: [] for key in pieces}
    for _ in range(reps):
        for key, fn in pieces.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[key].append(a.elapsed_time(b))
    res = {"ring": name, "log2_degree": k, "log2_n": nv, "table_bytes": n * eb, "index_bytes": n * 8, "reps": reps,
           "launches": {"a_indexed": la, "b_tables": lb}, "outputs_per_launch": {"a_indexed": pa, "b_tables": pb}, "a_equals_b": same,
           "model_a_over_b": round(elems["a_indexed"] / elems["b_tables"], 4)}
    for key in pieces:
        med = statistics.median(ms[key])
        res[key] = {"ms_median": round(med, 4), "ms_min": round(min(ms[key]), 4), "ms_max": round(max(ms[key]), 4), "elems": elems[key],
                    "tb_per_s": round(elems[key] * eb / (med * 1e-3) / 1e12, 3)}
    res["a_over_b"] = spread([x / y for x, y in zip(ms["a_indexed"], ms["b_tables"])])
    res["b_spread"] = round((max(ms["b_tables"]) - min(ms["b_tables"])) / statistics.median(ms["b_tables"]), 4)
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
            print("bench_index: %s 2^%d x 2^%d ran past %d s; stopping" % (name, k, nv, args.timeout), file=sys.stderr)
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
