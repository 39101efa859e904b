"""Times the product tree of a table on the GPU (DESIGN_APPENDIX.md A.14; raw output: profiles/prod_tree/).

For each table shape, in one child process per shape (each under its own time limit) and alternating per repetition:
  (a)  the new call, sr_prod_tree_dev, in both orders;
  (b)  the composition a caller had before it, trailing order only (the operands of the leading order are stride-2 views): per level
       a device copy of the lower half of the layer below into the layer, then sr_pointwise_mul_batch_dev by the upper half;
  (c)  sr_product_batch_dev alone: the cost of the root without any layer;
  (d)  add_dev on the two halves of the table: the streaming rate of the box in this run.
Device events sit around every timed piece; every shape is warmed up first, and before any time counts (a) trailing is compared bit
for bit with (b), and the roots of (a) in both orders with (c).  `bytes` is the traffic model of the piece for a table of n elements:
n * 8/7 read plus n - 1 written for (a) (each launch of three levels reads its input once and writes 7/8 of it), 5 (n - 1) for (b)
(per level of h outputs: h read and h written by the copy, 2 h read and h written by the product), n for (c), 1.5 n for (d).
The ratio (a)/(b) is taken per repetition; the spread of (b) is the margin.  Prints one JSON line per shape.

    python tools/bench_prod_tree.py [--reps 10] [--small] [--out FILE] [--timeout 240]
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

    from stark_rings_amd import CyclotomicRing

    assert torch.cuda.is_available(), "bench_prod_tree needs a GPU"
    ring = CyclotomicRing(name, k, device=0)
    w = ring.words_per_elem
    eb, n = w * 8, 1 << nv
    new = lambda elems: torch.empty(elems * w, dtype=torch.int64, device="cuda")  # noqa: E731
    leaves = new(n)
    ring.fill_uniform_dev(leaves, 0x9700, 0)
    out = {key: new(n - 1) for key in ("a_leading", "a_trailing", "b")}
    root = new(1)
    scratch = new(n // 2)
    offset = lambda lvl: ((1 << nv) - (1 << (nv - lvl + 1))) * w  # noqa: E731

    def run_b():
        below = leaves
        for lvl in range(1, nv + 1):
            half = (1 << (nv - lvl)) * w
            layer = out["b"][offset(lvl):offset(lvl) + half]
            layer.copy_(below[:half])
            ring.ntt_mul_dev(layer, below[half:2 * half])
            below = layer

    pieces = {"a_leading": lambda: ring.prod_tree_dev(out["a_leading"], leaves, nv, LEADING),
              "a_trailing": lambda: ring.prod_tree_dev(out["a_trailing"], leaves, nv, TRAILING),
              "b_copy_and_pointwise": run_b,
              "c_product_only": lambda: ring.product_dev(root, leaves),
              "d_add": lambda: ring.add_dev(scratch, leaves[:(n // 2) * w])}
    model = (n * 8 // 7 + n - 1) * eb
    nbytes = {"a_leading": model, "a_trailing": model, "b_copy_and_pointwise": 5 * (n - 1) * eb, "c_product_only": n * eb, "d_add": 3 * (n // 2) * eb}
    scratch.zero_()
    for f in pieces.values():
        f()
        f()
    torch.cuda.synchronize()
    same = {"a_trailing_equals_b": bool(torch.equal(out["a_trailing"], out["b"])),
            "root_leading_equals_c": bool(torch.equal(out["a_leading"][-w:], root)),
            "root_trailing_equals_c": bool(torch.equal(out["a_trailing"][-w:], root))}
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
    res = {"ring": name, "log2_degree": k, "num_vars": nv, "table_bytes": n * eb, "reps": reps, "launches": ring.prod_tree_plan(nv, TRAILING)[1],
           "launches_b": 2 * nv}
    res.update(same)
    for key in pieces:
        med = statistics.median(ms[key])
        res[key] = {"ms_median": round(med, 4), "ms_min": round(min(ms[key]), 4), "ms_max": round(max(ms[key]), 4), "bytes": nbytes[key],
                    "tb_per_s": round(nbytes[key] / (med * 1e-3) / 1e12, 3)}
    res["a_trailing_over_b"] = spread([x / y for x, y in zip(ms["a_trailing"], ms["b_copy_and_pointwise"])])
    res["a_leading_over_b"] = spread([x / y for x, y in zip(ms["a_leading"], ms["b_copy_and_pointwise"])])
    res["a_trailing_over_c"] = spread([x / y for x, y in zip(ms["a_trailing"], ms["c_product_only"])])
    med_b = statistics.median(ms["b_copy_and_pointwise"])
    res["b_spread"] = round((max(ms["b_copy_and_pointwise"]) - min(ms["b_copy_and_pointwise"])) / med_b, 4)
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
            print("bench_prod_tree: %s 2^%d x 2^%d ran past %d s; stopping" % (name, k, nv, args.timeout), file=sys.stderr)
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
