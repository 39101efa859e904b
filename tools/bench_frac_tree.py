"""Times the fraction tree of two tables on the GPU (DESIGN_APPENDIX.md A.15; raw output: profiles/frac_tree/).

For each table shape, in one child process per shape (each under its own time limit) and alternating per repetition:
  (a)  the new call, sr_frac_tree_dev, in both orders, with and without stored numerators;
  (b)  the composition a caller had before it, trailing order only (the operands of the leading order are stride-2 views): per level,
       on the q side a device copy of q_lo into the layer and sr_pointwise_mul_batch_dev by q_hi; on the p side a copy of p_lo into
       the layer and a product by q_hi, a copy of p_hi into a temporary and a product by q_lo, and sr_add_batch_dev of the two;
  (c)  sr_prod_tree_dev of the q leaves alone: the q side without any numerator;
  (d)  add_dev on the two halves of a table: the streaming rate of the box in this run.
Device events sit around every timed piece; every shape is warmed up first, and before any time counts (a) trailing is compared bit
for bit with (b), and the q layers of (a) with (c).  `bytes` is the traffic model of the piece for tables of n elements and J levels
per launch: 2 n / (1 - 2^-J) read plus 2 (n - 1) written for (a) (4.3 n for J = 3, 4.7 n for J = 2; n / (1 - 2^-J) less read by the
first launch where no numerators are stored), 18 (n - 1) for (b) (per level of h outputs 5 h on the q side and 13 h on the p side),
the model of tools/bench_prod_tree.py for (c), 1.5 n for (d).  The ratio (a)/(b) is taken per repetition; the spread of (b) is the
margin.  Prints one JSON line per shape.

    python tools/bench_frac_tree.py [--reps 10] [--small] [--out FILE] [--timeout 240]
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
LEADING, TRAILING = 0, 1


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def run_shape(name, k, nv, reps):
    import torch

    from stark_rings_amd import CyclotomicRing, frac_tree_dev, frac_tree_plan

    assert torch.cuda.is_available(), "bench_frac_tree needs a GPU"
    ring = CyclotomicRing(name, k, device=0)
    w = ring.words_per_elem
    eb, n = w * 8, 1 << nv
    new = lambda elems: torch.empty(elems * w, dtype=torch.int64, device="cuda")  # noqa: E731
    p_leaves, q_leaves = new(n), new(n)
    ring.fill_uniform_dev(p_leaves, 0x9800, 0)
    ring.fill_uniform_dev(q_leaves, 0x9801, 0)
    keys = ("a_leading", "a_trailing", "a_leading_no_numerators", "a_trailing_no_numerators", "b")
    out_p = {key: new(n - 1) for key in keys}
    out_q = {key: new(n - 1) for key in keys}
    prod = new(n - 1)
    tmp = new(n // 2)
    scratch = new(n // 2)
    offset = lambda lvl: ((1 << nv) - (1 << (nv - lvl + 1))) * w  # noqa: E731

    def run_b():
        below_p, below_q = p_leaves, q_leaves
        for lvl in range(1, nv + 1):
            half = (1 << (nv - lvl)) * w
            lp = out_p["b"][offset(lvl):offset(lvl) + half]
            lq = out_q["b"][offset(lvl):offset(lvl) + half]
            t = tmp[:half]
            lp.copy_(below_p[:half])
            ring.ntt_mul_dev(lp, below_q[half:2 * half])
            t.copy_(below_p[half:2 * half])
            ring.ntt_mul_dev(t, below_q[:half])
            ring.add_dev(lp, t)
            lq.copy_(below_q[:half])
            ring.ntt_mul_dev(lq, below_q[half:2 * half])
            below_p, below_q = lp, lq

    def run_a(key, numer, order):
        return lambda: frac_tree_dev(ring, out_p[key], out_q[key], p_leaves if numer else None, q_leaves, nv, order)

    pieces = {"a_leading": run_a("a_leading", True, LEADING), "a_trailing": run_a("a_trailing", True, TRAILING),
              "a_leading_no_numerators": run_a("a_leading_no_numerators", False, LEADING),
              "a_trailing_no_numerators": run_a("a_trailing_no_numerators", False, TRAILING),
              "b_composition": run_b,
              "c_prod_tree_of_q": lambda: ring.prod_tree_dev(prod, q_leaves, nv, TRAILING),
              "d_add": lambda: ring.add_dev(scratch, q_leaves[:(n // 2) * w])}
    launches = frac_tree_plan(ring, nv, TRAILING)[1]
    j = -(-nv // launches)   # levels per full launch
    read = 2 * n * (1 << j) // ((1 << j) - 1)
    model = (read + 2 * (n - 1)) * eb
    model_no = model - n * eb
    jp = -(-nv // ring.prod_tree_plan(nv, TRAILING)[1])
    nbytes = {"a_leading": model, "a_trailing": model, "a_leading_no_numerators": model_no, "a_trailing_no_numerators": model_no,
              "b_composition": 18 * (n - 1) * eb, "c_prod_tree_of_q": (n * (1 << jp) // ((1 << jp) - 1) + n - 1) * eb, "d_add": 3 * (n // 2) * eb}
    scratch.zero_()
    for f in pieces.values():
        f()
        f()
    torch.cuda.synchronize()
    same = {"a_trailing_equals_b": bool(torch.equal(out_p["a_trailing"], out_p["b"]) and torch.equal(out_q["a_trailing"], out_q["b"])),
            "q_trailing_equals_c": bool(torch.equal(out_q["a_trailing"], prod) and torch.equal(out_q["a_trailing_no_numerators"], prod)),
            "roots_of_both_orders_agree": bool(torch.equal(out_p["a_leading"][-w:], out_p["a_trailing"][-w:])
                                               and torch.equal(out_q["a_leading"][-w:], out_q["a_trailing"][-w:])
                                               and torch.equal(out_p["a_leading_no_numerators"][-w:], out_p["a_trailing_no_numerators"][-w:]))}
    assert all(same.values()), same   # no time counts unless every variant agrees bit for bit
    ms = {key: [] for key in pieces}
    for _ in range(reps):
        for key, f in pieces.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[key].append(a.elapsed_time(b))
    res = {"ring": name, "log2_degree": k, "num_vars": nv, "table_bytes": n * eb, "reps": reps, "launches": launches, "levels_per_launch": j,
           "launches_b": 7 * nv, "model_a_over_b": round(model / nbytes["b_composition"], 4)}
    res.update(same)
    for key in pieces:
        med = statistics.median(ms[key])
        res[key] = {"ms_median": round(med, 4), "ms_min": round(min(ms[key]), 4), "ms_max": round(max(ms[key]), 4), "bytes": nbytes[key],
                    "tb_per_s": round(nbytes[key] / (med * 1e-3) / 1e12, 3)}
    for key in ("a_trailing", "a_leading", "a_trailing_no_numerators", "a_leading_no_numerators"):
        res[key + "_over_b"] = spread([x / y for x, y in zip(ms[key], ms["b_composition"])])
    res["a_trailing_over_c"] = spread([x / y for x, y in zip(ms["a_trailing"], ms["c_prod_tree_of_q"])])
    res["no_numerators_over_a_trailing"] = spread([x / y for x, y in zip(ms["a_trailing_no_numerators"], ms["a_trailing"])])
    med_b = statistics.median(ms["b_composition"])
    res["b_spread"] = round((max(ms["b_composition"]) - min(ms["b_composition"])) / med_b, 4)
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
            print("bench_frac_tree: %s 2^%d x 2^%d ran past %d s; stopping" % (name, k, nv, args.timeout), file=sys.stderr)
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
