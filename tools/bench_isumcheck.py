"""Times the first message and the fused first fold of a weighted sum-check whose selectors are integer columns (DESIGN_APPENDIX.md
A.21; raw output: profiles/isumcheck/), in one process per shape:
  (a)  the columns read as u64: sr_vpoly_iwround_evals_dev, then sr_vpoly_iwround_fold_evals_dev;
  (b)  the existing weighted calls over tables ALREADY expanded (sr_vpoly_wround_evals_dev, sr_vpoly_wround_fold_evals_dev): the code
       path before integer columns, the expansion not counted;
  (c)  (b) plus the from_u64_dev expansion of every column, which is what a caller of (b) pays in full.
PLONK is  q_L a + q_R b + q_M a b - q_O c + q_C  (3 tables, 5 selector columns of 0/1: the 8-slot kernels); ALLCOL one product of two
columns.  Every buffer is allocated before anything is timed.  A warm-up of every variant, the message, the fused message and every
folded slot of (a) and (b) compared bit for bit before any time counts, then the variants alternating per repetition with device
events around every piece.  The ratio (a) / (b) is taken per repetition; the spread of (b) over its repeats is the margin.  `model` is
the traffic of A.21 in table sizes: message (K + 0.25) / (K + J + 0.25), fold (K + (K + J) / 2) / ((K + J) 1.5).  Prints one JSON line
per shape.

    python tools/bench_isumcheck.py [--reps 10] [--small] [--out FILE] [--timeout 400]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("PLONK", "goldilocks", 16, 8), ("PLONK", "goldilocks", 10, 14), ("PLONK", "babybear", 16, 8), ("PLONK", "stark", 12, 8),
          ("PLONK", "goldilocks24", 0, 20), ("ALLCOL", "goldilocks", 10, 14)]
SMALL = [("PLONK", "goldilocks", 16, 4), ("PLONK", "goldilocks", 10, 8), ("PLONK", "babybear", 16, 4), ("PLONK", "stark", 12, 4),
         ("PLONK", "goldilocks24", 0, 12), ("ALLCOL", "goldilocks", 10, 8)]
STRUCTURES = {"PLONK": (3, 5, [[3, 0], [4, 1], [5, 0, 1], [6, 2], [7]]), "ALLCOL": (0, 2, [[0, 1]])}
TRAILING = 1


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def run_shape(sname, name, k, nv, reps):
    import torch

    from stark_rings_amd import (CyclotomicRing, IndexColumn, from_u64_dev, vpoly_iwround_evals_dev, vpoly_iwround_fold_evals_dev,
                                 vpoly_iwround_plan, vpoly_wround_evals_dev, vpoly_wround_fold_evals_dev)

    assert torch.cuda.is_available(), "bench_isumcheck needs a GPU"
    ring = CyclotomicRing(name, k, device=0)
    w, full, order = ring.words_per_elem, 1 << nv, TRAILING
    K, J, terms = STRUCTURES[sname]
    d = max(len(t) for t in terms)
    new = lambda elems: torch.empty(elems * w, dtype=torch.int64, device="cuda")  # noqa: E731
    tables = [new(full) for _ in range(K)]
    for j, t in enumerate(tables):
        ring.fill_uniform_dev(t, 0x15C00 + j, 0)
    gen = torch.Generator(device="cuda").manual_seed(0x15C)
    cols = [IndexColumn(torch.randint(0, 2, (full,), dtype=torch.int64, device="cuda", generator=gen)) for _ in range(J)]
    wts, wtf, r, coeffs = new(full // 2), new(full // 4), new(1), new(len(terms))
    for j, t in enumerate((wts, wtf, r, coeffs)):
        ring.fill_uniform_dev(t, 0x15D00 + j, 0)
    dense = [new(full) for _ in range(J)]
    msg = {v: new(d + 1) for v in "ab"}
    fmsg = {v: new(d + 1) for v in "ab"}
    folded = {v: [new(full // 2) for _ in range(K + J)] for v in "ab"}
    plans = {"a": (vpoly_iwround_plan(ring, nv, K, J, len(terms), d, order)[0], vpoly_iwround_plan(ring, nv, K, J, len(terms), d, order, fold=True)[0]),
             "b": (ring.vpoly_wround_plan(nv, K + J, len(terms), d, order)[0], ring.vpoly_wround_fold_plan(nv, K + J, len(terms), d, order)[0])}
    work = {v: [new(n) if n else None for n in plans[v]] for v in "ab"}

    def expand():
        for c, out in zip(cols, dense):
            from_u64_dev(ring, c, full, out=out)

    def run_a():
        vpoly_iwround_evals_dev(ring, msg["a"], wts, tables, cols, terms, coeffs, nv, order, work["a"][0])
        vpoly_iwround_fold_evals_dev(ring, fmsg["a"], folded["a"], wtf, tables, cols, terms, coeffs, nv, r, order, work["a"][1])

    def run_b():
        vpoly_wround_evals_dev(ring, msg["b"], wts, tables + dense, terms, coeffs, nv, order, work["b"][0])
        vpoly_wround_fold_evals_dev(ring, fmsg["b"], folded["b"], wtf, tables + dense, terms, coeffs, nv, r, order, work["b"][1])

    def run_c():
        expand()
        run_b()

    pieces = {"a_columns_as_u64": run_a, "b_expanded_tables": run_b, "c_expansion_and_b": run_c}
    for _ in range(2):
        run_c()
        run_a()
    torch.cuda.synchronize()
    same = bool(torch.equal(msg["a"], msg["b"])) and bool(torch.equal(fmsg["a"], fmsg["b"])) and \
        all(bool(torch.equal(x, y)) for x, y in zip(folded["a"], folded["b"]))
    ms = {key: [] for key in pieces}
    if same:
        for _ in range(reps):
            for key, f in pieces.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                ms[key].append(a.elapsed_time(b))
    T = K + J
    res = {"structure": sname, "ring": name, "log2_degree": k, "num_vars": nv, "order": "trailing", "reps": reps, "tables": K, "columns": J,
           "table_bytes": full * w * 8, "a_equals_b": same,
           "model": {"message": round((K + 0.25) / (T + 0.25), 4), "fold": round((K + T / 2) / (T * 1.5), 4),
                     "both": round((2 * K + 0.25 + T / 2) / (T + 0.25 + T * 1.5), 4)}}
    if same:
        for key in pieces:
            res[key] = {"ms_median": round(statistics.median(ms[key]), 4), "ms_min": round(min(ms[key]), 4), "ms_max": round(max(ms[key]), 4)}
        res["a_over_b"] = spread([x / y for x, y in zip(ms["a_columns_as_u64"], ms["b_expanded_tables"])])
        res["a_over_c"] = spread([x / y for x, y in zip(ms["a_columns_as_u64"], ms["c_expansion_and_b"])])
        med_b = statistics.median(ms["b_expanded_tables"])
        res["b_spread"] = spread([x / med_b for x in ms["b_expanded_tables"]])
    print(json.dumps(res), flush=True)
    ring.close()
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="tables 2^4 to 2^8 times smaller (a quick check of the tool itself)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=400, help="seconds one shape's child process may take")
    ap.add_argument("--shape", default=None, help="(internal) structure,ring,log2_degree,num_vars: run this shape in this process")
    args = ap.parse_args()
    if args.shape:
        sname, name, k, nv = args.shape.split(",")
        return run_shape(sname, name, int(k), int(nv), args.reps)
    lines = []
    for sname, name, k, nv in (SMALL if args.small else SHAPES):
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--shape", "%s,%s,%d,%d" % (sname, name, k, nv)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("bench_isumcheck: %s %s 2^%d x 2^%d ran past %d s; stopping" % (sname, name, k, nv, args.timeout), file=sys.stderr)
            return 124
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if args.out and lines:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        if r.returncode != 0:  # a failed step ends the run: nothing more is started on the device
            sys.stderr.write(r.stderr)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
