"""Times a whole sum-check -- all rounds -- of the two layer claims of the layered (GKR) arguments, over the top layer (layer 1: the
halves of the leaves) of a trailing-order tree, with and without an eq table (DESIGN_APPENDIX.md A.16; raw output: profiles/eq_sumcheck/):
  (i)  L_1(z) = sum_b eq(z, b) lo(b) hi(b)                                                       (ProductTree)
  (ii) P_1(z) + lambda Q_1(z) = sum_b eq(z, b) (p_lo q_hi + p_hi q_lo + lambda q_lo q_hi)(b)    (FractionTree)
each as
  (a)  EqSumCheck: eq(z, .) as per-pair weights (sr_vpoly_wround_evals_dev, sr_vpoly_wround_fold_evals_dev); the weights of all
       rounds are built inside the timed piece, and so are message() and next() of every round;
  (b)  the explicit path, the way of the code before: the eq table (sr_eq_table_dev, inside the timed piece) as one more table slot of
       every product, sr_vpoly_round_evals_dev, then sr_vpoly_round_fold_evals_dev per round;
  (c)  add_dev on the two halves of one table: the streaming rate of the box in this run.
One child process per shape (each under its own time limit), a warm-up of every variant, the messages of all rounds and the final
values of (a) and (b) compared bit for bit before any time counts, then the variants alternating per repetition with device events
around every piece.  The ratio (a) / (b) is taken per repetition; the spread of (b) is the margin.  `model` is the ratio of the
traffic-and-points model of A.16 for one fused round: (tables + 0.25) / (tables + 1) * 1.5 n of traffic, (d + 1) / (d + 2) points.
Prints one JSON line per (shape, claim).

    python tools/bench_wsumcheck.py [--reps 10] [--small] [--out FILE] [--timeout 400]
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
TRAILING = 1
# per fused round in units of the table size entering the round: 1.5 per table; the eq factor 1.5 as a table, 0.25 as weights
MODEL = {"product": {"traffic": (2 * 1.5 + 0.25) / (3 * 1.5), "points": 3 / 4}, "fraction": {"traffic": (4 * 1.5 + 0.25) / (5 * 1.5), "points": 3 / 4}}


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def run_shape(name, k, nv, reps):
    import torch

    from stark_rings_amd import CyclotomicRing, DenseMultilinearExtension as MLE, EqSumCheck, FractionTree, ProductTree, VirtualPolynomial

    assert torch.cuda.is_available(), "bench_wsumcheck needs a GPU"
    ring = CyclotomicRing(name, k, device=0)
    w = ring.words_per_elem
    new = lambda elems: torch.empty(elems * w, dtype=torch.int64, device="cuda")  # noqa: E731
    q_leaves, p_leaves = new(1 << nv), new(1 << nv)
    ring.fill_uniform_dev(q_leaves, 0x5E00, 0)
    ring.fill_uniform_dev(p_leaves, 0x5E01, 0)
    n = nv - 1  # variables of the claim over the halves of the leaves
    z, lam, rs = new(n), new(1), new(n)
    ring.fill_uniform_dev(z, 0x5E02, 0)
    ring.fill_uniform_dev(lam, 0x5E03, 0)
    ring.fill_uniform_dev(rs, 0x5E04, 0)
    challenges = [rs[j * w:(j + 1) * w] for j in range(n)]
    for claim in ("product", "fraction"):
        tree = ProductTree(ring, q_leaves, nv) if claim == "product" else FractionTree(ring, p_leaves, q_leaves, nv)
        halves = tree.halves(1)

        def poly():
            g = VirtualPolynomial(ring, n)
            if claim == "product":
                return g.add_mle_list(list(halves))
            p_lo, p_hi, q_lo, q_hi = halves
            return g.add_mle_list([p_lo, q_hi]).add_mle_list([p_hi, q_lo]).add_mle_list([q_lo, q_hi], lam)

        def run_a():
            prover = EqSumCheck(poly(), z, TRAILING)
            msgs = []
            for j in range(n):
                msgs.append(prover.message())
                prover.next(challenges[j])
            finals, eq_r = prover.final()
            return msgs, list(finals) + [eq_r]

        def run_b():
            e = poly().mul_by_mle(MLE.eq(ring, z))
            msgs = [e.round_evals(TRAILING)]
            for j in range(n - 1):
                msg, e = e.fold_round_evals(challenges[j], TRAILING)
                msgs.append(msg)
            e = e.fixed_variables(challenges[n - 1], TRAILING)
            return msgs, [t.evaluations for t in e.tables]

        half = halves[0].evaluations
        scratch = torch.empty_like(half)
        pieces = {"a_eq_sumcheck": run_a, "b_explicit_eq_table": run_b, "c_add": lambda: ring.add_dev(scratch, half)}
        for _ in range(2):
            got_a, got_b = run_a(), run_b()
        torch.cuda.synchronize()
        same = all(bool(torch.equal(x, y)) for x, y in zip(got_a[0] + got_a[1], got_b[0] + got_b[1])) and len(got_a[0]) == len(got_b[0]) == n
        del got_a, got_b
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
        res = {"ring": name, "log2_degree": k, "num_vars": nv, "claim": claim, "rounds": n, "order": "trailing", "reps": reps,
               "table_bytes": half.numel() * 8, "tables": len(halves), "a_equals_b": same, "model": MODEL[claim]}
        if same:
            for key in pieces:
                med = statistics.median(ms[key])
                res[key] = {"ms_median": round(med, 4), "ms_min": round(min(ms[key]), 4), "ms_max": round(max(ms[key]), 4)}
            res["c_add"]["tb_per_s"] = round(3 * half.numel() * 8 / (statistics.median(ms["c_add"]) * 1e-3) / 1e12, 3)
            res["a_over_b"] = spread([x / y for x, y in zip(ms["a_eq_sumcheck"], ms["b_explicit_eq_table"])])
            med_b = statistics.median(ms["b_explicit_eq_table"])
            res["b_spread"] = spread([x / med_b for x in ms["b_explicit_eq_table"]])
        print(json.dumps(res), flush=True)
        del tree, halves, half, scratch
        if not same:
            ring.close()
            return 1
    ring.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="tables 2^6 times smaller (a quick check of the tool itself)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=400, help="seconds one shape's child process may take")
    ap.add_argument("--shape", default=None, help="(internal) ring,log2_degree,num_vars: run this shape in this process")
    args = ap.parse_args()
    if args.shape:
        name, k, nv = args.shape.split(",")
        return run_shape(name, int(k), int(nv), args.reps)
    lines = []
    for name, k, nv in (SMALL if args.small else TABLES):
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--shape", "%s,%d,%d" % (name, k, nv)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("bench_wsumcheck: %s 2^%d x 2^%d ran past %d s; stopping" % (name, k, nv, args.timeout), file=sys.stderr)
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
