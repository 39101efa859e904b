"""Times the sum-check round message of a sum of products on the GPU (DESIGN_APPENDIX.md A.11; raw output: profiles/vpoly/).

For each table shape, in one child process per shape (each under its own time limit) and alternating per repetition:
  (a) the new call on R1CS, c0 e a b - e c, leading order: sr_vpoly_round_evals_dev, four tables read once, all four points;
  (b) the same message from the entry points that existed before it: sr_mle_round_evals_dev(e, a, b) and sr_mle_round_evals_dev(e, c)
      (five table reads), the fourth point of the degree-2 term by p(3) = p(0) - 3 p(1) + 3 p(2) on single elements (sub_dev, add_dev),
      the two messages scaled by their coefficients (mul_elem_dev) and added (add_dev);
  (c) a single product of three tables without coefficients through the new call, against sr_mle_round_evals_dev on the same
      tables: the price of the runtime term walk;
  (d) add_dev on the two halves of one table: the streaming rate of the box in this run.
Device events sit around every timed piece; every shape is warmed up first.  Prints one JSON line per shape.

    python tools/bench_vpoly.py [--reps 10] [--small] [--out FILE] [--timeout 240]
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
R1CS = [[0, 1, 2], [0, 3]]
SINGLE = [[0, 1, 2]]


def run_shape(name, k, nv, reps):
    import torch

    from stark_rings_amd import CyclotomicRing

    assert torch.cuda.is_available(), "bench_vpoly needs a GPU"
    ring = CyclotomicRing(name, k, device=0)
    w = ring.words_per_elem
    eb, n = w * 8, 1 << nv
    tables = []
    for j in range(4):  # e, a, b, c
        t = torch.empty(n * w, dtype=torch.int64, device="cuda")
        ring.fill_uniform_dev(t, 0x7C00 + j, 0)
        tables.append(t)
    e, a, b, c = tables
    coeffs = torch.empty(2 * w, dtype=torch.int64, device="cuda")
    ring.fill_uniform_dev(coeffs[:w], 0x7C10, 0)
    ring.eq_table_dev(coeffs[w:], None)
    ring.neg_dev(coeffs[w:])  # c1 = -one()
    c0, c1 = coeffs[:w].clone(), coeffs[w:].clone()

    def workspace(elems):
        return torch.empty(max(elems, 1) * w, dtype=torch.int64, device="cuda") if elems else None

    need_a, launches_a = ring.vpoly_round_plan(nv, 4, 2, 3, LEADING)
    need_s, launches_s = ring.vpoly_round_plan(nv, 3, 1, 3, LEADING)
    need_3, launches_3 = ring.mle_round_plan(nv, 3, LEADING)
    need_2, _ = ring.mle_round_plan(nv, 2, LEADING)
    work_a, work_s, work_3, work_2 = workspace(need_a), workspace(need_s), workspace(need_3), workspace(need_2)
    out_a = torch.empty(4 * w, dtype=torch.int64, device="cuda")
    m1 = torch.empty(4 * w, dtype=torch.int64, device="cuda")
    m2 = torch.empty(4 * w, dtype=torch.int64, device="cuda")
    diff = torch.empty(w, dtype=torch.int64, device="cuda")
    out_s = torch.empty(4 * w, dtype=torch.int64, device="cuda")
    out_r = torch.empty(4 * w, dtype=torch.int64, device="cuda")
    lo, hi = torch.empty((n // 2) * w, dtype=torch.int64, device="cuda"), torch.empty((n // 2) * w, dtype=torch.int64, device="cuda")

    def run_a():
        ring.vpoly_round_evals_dev(out_a, tables, R1CS, coeffs, nv, LEADING, work_a)

    def run_b():
        ring.mle_round_evals_dev(m1, [e, a, b], nv, LEADING, work_3)
        ring.mle_round_evals_dev(m2[:3 * w], [e, c], nv, LEADING, work_2)
        # p(3) = p(0) + 3 (p(2) - p(1))
        diff.copy_(m2[2 * w:3 * w])
        ring.sub_dev(diff, m2[w:2 * w])
        m2[3 * w:].copy_(m2[:w])
        for _ in range(3):
            ring.add_dev(m2[3 * w:], diff)
        ring.mul_elem_dev(m1, c0)
        ring.mul_elem_dev(m2, c1)
        ring.add_dev(m1, m2)

    def run_c_new():
        ring.vpoly_round_evals_dev(out_s, tables[:3], SINGLE, None, nv, LEADING, work_s)

    def run_c_old():
        ring.mle_round_evals_dev(out_r, tables[:3], nv, LEADING, work_3)

    def run_d():
        ring.add_dev(lo, hi)

    pieces = {"a_vpoly_r1cs": run_a, "b_composed_r1cs": run_b, "c_vpoly_single": run_c_new, "c_round_single": run_c_old, "d_add": run_d}
    half = (n // 2) * eb
    nbytes = {"a_vpoly_r1cs": 4 * n * eb, "b_composed_r1cs": 5 * n * eb, "c_vpoly_single": 3 * n * eb, "c_round_single": 3 * n * eb, "d_add": 3 * half}
    for f in pieces.values():
        f()
        f()
    torch.cuda.synchronize()
    same_r1cs = bool(torch.equal(out_a, m1))
    same_single = bool(torch.equal(out_s, out_r))
    ms = {key: [] for key in pieces}
    for _ in range(reps):
        for key, f in pieces.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            t1.synchronize()
            ms[key].append(t0.elapsed_time(t1))
    res = {"ring": name, "log2_degree": k, "num_vars": nv, "table_bytes": n * eb, "reps": reps, "launches_r1cs": launches_a,
           "launches_single": launches_s, "launches_round_d3": launches_3, "work_elems_r1cs": need_a, "vpoly_equals_composed": same_r1cs,
           "single_equals_round": same_single}
    for key in pieces:
        med = statistics.median(ms[key])
        res[key] = {"ms_median": round(med, 4), "ms_min": round(min(ms[key]), 4), "ms_max": round(max(ms[key]), 4), "bytes": nbytes[key],
                    "tb_per_s": round(nbytes[key] / (med * 1e-3) / 1e12, 3)}
    # per repetition, so that the spread of a ratio is that of one run beside the other
    ab = [x / y for x, y in zip(ms["a_vpoly_r1cs"], ms["b_composed_r1cs"])]
    cc = [x / y for x, y in zip(ms["c_vpoly_single"], ms["c_round_single"])]
    for key, r in (("a_over_b", ab), ("c_new_over_old", cc)):
        res[key] = {"median": round(statistics.median(r), 4), "min": round(min(r), 4), "max": round(max(r), 4)}
    bm = res["b_composed_r1cs"]
    res["b_spread"] = round((bm["ms_max"] - bm["ms_min"]) / bm["ms_median"], 4)  # the margin: only a_over_b below 1 by more is a gain
    res["a_share_of_add_rate"] = round(res["a_vpoly_r1cs"]["tb_per_s"] / res["d_add"]["tb_per_s"], 3)
    print(json.dumps(res), flush=True)
    ring.close()
    return res


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
            print("bench_vpoly: %s 2^%d x 2^%d ran past %d s; stopping" % (name, k, nv, args.timeout), file=sys.stderr)
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
