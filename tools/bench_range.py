"""Times the range-check (norm-check) rounds (DESIGN_APPENDIX.md A.18; raw output: profiles/range_check/).

bound 2 -- a whole sum-check, all rounds, of  sum_b eq(z, b) P_2(f(b))  over one witness table, trailing order, as
  (a)  EqSumCheck(RangePolynomial): sr_range_wround_evals_dev per round and sr_mle_fix_variables_dev of one table between rounds;
  (b)  the only way of the code before: two add_scalar_dev passes (f - 1, f + 1; copies and passes inside the timed piece), then
       EqSumCheck over the VirtualPolynomial of three table slots -- sr_vpoly_wround_evals_dev, then sr_vpoly_wround_fold_evals_dev
       per round, which reads and folds three tables;
  (c)  add_dev on the two halves of the table: the streaming rate of the box in this run.
The messages of all rounds and the final values of (a) and (b) are compared bit for bit before any time counts; then the variants
alternate per repetition with device events around every piece.  The ratio (a) / (b) is taken per repetition; the spread of (b),
(max - min) / median, is the margin: (a) counts as faster only where the gain exceeds it.  The kernels of (b) are the entry points the
library had before this call; none of them, and no header they share, differs from the parent's, so (b) is timed in the same process.

bound 3, 5, 8 -- there is no one-call yardstick.  Per bound: the time of the first round's call over one table (all its launches),
beside the streaming time of ONE read of the table and the weights at the rate of (c), and the VALU-issue floor of the listing: per
point and unit B canonical products (the square and the B - 1 shifted factors) of L VALU instructions each -- L is the body of the
run-time loop over the shifts in the gfx950 listing, tests/test_range_isa.py; the lazy term and the running sum are left out -- at
4.25 cycles per wave-instruction and SIMD (profiles/r01/valu_issue_rates_gfx950.txt) and the nominal 2.4 GHz over 256 x 4 SIMDs.

One child process per shape (each under its own time limit).  Prints one JSON line per (shape, bound).

    python tools/bench_range.py [--reps 12] [--small] [--out FILE] [--timeout 300]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (ring, log2 D, num_vars): 2 GiB per table for the one-limb fields, 512 MiB for Stark, 1.5 GiB for goldilocks24 (the shapes of A.17)
TABLES = [("goldilocks", 16, 12), ("babybear", 16, 12), ("stark", 12, 12), ("goldilocks24", 0, 23)]
SMALL = [("goldilocks", 16, 6), ("babybear", 16, 6), ("stark", 12, 6), ("goldilocks24", 0, 14)]
TRAILING = 1
# VALU instructions of one canonical product with its shift (the loop body of the listing), units per element as the kernel maps
# them with 16-byte-aligned tables (a pair of coefficients, one Stark coefficient, one slot), products per unit and loop body
LOOP_VALU = {"goldilocks": 24, "babybear": 12, "stark": 324, "goldilocks24": 242, "babybear72": 434, "frog16": 939}
PER_UNIT = {"goldilocks": 2, "babybear": 2, "stark": 1, "goldilocks24": 1, "babybear72": 1, "frog16": 1}
PER_LAUNCH = {"goldilocks": 7, "babybear": 8, "stark": 3, "goldilocks24": 2, "babybear72": 2, "frog16": 2}
CYCLES_PER_WAVE_INSTR, CLOCK_HZ, SIMDS = 4.25, 2.4e9, 256 * 4


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def run_shape(name, k, nv, reps):
    import torch

    from stark_rings_amd import (CyclotomicRing, DenseMultilinearExtension as MLE, EqSumCheck, RangePolynomial, VirtualPolynomial,
                                 range_wround_evals_dev, range_wround_plan)

    assert torch.cuda.is_available(), "bench_range needs a GPU"
    ring = CyclotomicRing(name, k, device=0)
    w = ring.words_per_elem
    new = lambda elems: torch.empty(elems * w, dtype=torch.int64, device="cuda")  # noqa: E731
    f, z, rs, wts = new(1 << nv), new(nv), new(nv), new(1 << (nv - 1))
    for t, seed in ((f, 0x6E00), (z, 0x6E01), (rs, 0x6E02), (wts, 0x6E03)):
        ring.fill_uniform_dev(t, seed, 0)
    challenges = [rs[j * w:(j + 1) * w] for j in range(nv)]
    one = new(1)
    ring.eq_table_dev(one, None)
    # the images of +1 and -1 as add_scalar_dev takes them: component 0 of the first slot of one() and of -one()
    minus = one.clone()
    ring.neg_dev(minus)
    plus_img, minus_img = one[:ring.limbs].cpu().numpy().view("uint64"), minus[:ring.limbs].cpu().numpy().view("uint64")
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    def prove(g):
        prover = EqSumCheck(g, z, TRAILING)
        msgs = []
        for j in range(nv):
            msgs.append(prover.message())
            prover.next(challenges[j])
        finals, eq_r = prover.final()
        return msgs, finals, eq_r

    def run_a():
        return prove(RangePolynomial(ring, [MLE(ring, nv, f)], 2))

    def run_b():
        lo, hi = f.clone(), f.clone()
        ring.add_scalar_dev(lo, minus_img, True)
        ring.add_scalar_dev(hi, plus_img, True)
        g = VirtualPolynomial(ring, nv)
        g.add_mle_list([MLE(ring, nv, f), MLE(ring, nv, lo), MLE(ring, nv, hi)])
        return prove(g)

    half = f.numel() // 2
    scratch = f[:half].clone()

    def run_c():
        ring.add_dev(scratch, f[half:])

    (ma, fa, ea), (mb, fb, eb) = run_a(), run_b()  # warm-up and the comparison
    run_c()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(ma, mb)) and torch.equal(fa[0], fb[0]) and torch.equal(ea, eb), "bound 2: (a) and (b) differ"
    ta, tb, tc = [], [], []
    for _ in range(reps):
        ta.append(timed(run_a)[0])
        tb.append(timed(run_b)[0])
        tc.append(timed(run_c)[0])
    table_bytes = f.numel() * 8
    add_tbs = 1.5 * table_bytes / (statistics.median(tc) * 1e-3) / 1e12  # two halves read, one written
    ratios = [a / b for a, b in zip(ta, tb)]
    mb_ = statistics.median(tb)
    line = {"bench": "range_check", "ring": name, "log2_degree": k, "num_vars": nv, "bound": 2, "table_mib": table_bytes >> 20, "reps": reps,
            "a_ms": spread(ta), "b_ms": spread(tb), "add_tbs": round(add_tbs, 3), "ratio": spread(ratios),
            "spread_of_b": round((max(tb) - min(tb)) / mb_, 4)}
    line["faster"] = bool(1 - statistics.median(ratios) > line["spread_of_b"])
    print(json.dumps(line), flush=True)
    # the first round's call alone at larger bounds
    units = (ring.degree // 2 if name in ("goldilocks", "babybear") else ring.degree if name == "stark" else {"goldilocks24": 8, "babybear72": 8, "frog16": 4}[name])
    pairs = 1 << (nv - 1)
    for bound in (2, 3, 5, 8):
        out = new(2 * bound)
        work_elems, launches = range_wround_plan(ring, nv, 1, bound, TRAILING)
        work = new(work_elems) if work_elems else None
        call = lambda: range_wround_evals_dev(ring, out, wts, [f], bound, None, nv, TRAILING, work)  # noqa: E731
        call()
        torch.cuda.synchronize()
        tr = [timed(call)[0] for _ in range(reps)]
        stream_ms = 1.5 * table_bytes / (add_tbs * 1e12) * 1e3  # one read of the table and the weights
        wave_instr = pairs * units / 64 * PER_UNIT[name] * 2 * bound * bound * LOOP_VALU[name]
        valu_ms = wave_instr * CYCLES_PER_WAVE_INSTR / (SIMDS * CLOCK_HZ) * 1e3
        point_launches = -(-2 * bound // PER_LAUNCH[name])
        print(json.dumps({"bench": "range_check_round", "ring": name, "log2_degree": k, "num_vars": nv, "bound": bound, "launches": launches,
                          "point_launches": point_launches, "reps": reps, "round_ms": spread(tr), "stream_once_ms": round(stream_ms, 4),
                          "stream_all_launches_ms": round(stream_ms * point_launches, 4), "valu_floor_ms": round(valu_ms, 4),
                          "add_tbs": round(add_tbs, 3),
                          "nearer_bound": "valu" if valu_ms > stream_ms * point_launches else "stream"}), flush=True)
    ring.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_check", "bench_range.jsonl"))
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--shape", default=None, help="internal: ring,log2_degree,num_vars of a child process")
    args = ap.parse_args()
    if args.shape:
        name, k, nv = args.shape.split(",")
        run_shape(name, int(k), int(nv), args.reps)
        return 0
    lines = []
    for name, k, nv in (SMALL if args.small else TABLES):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--shape", "%s,%d,%d" % (name, k, nv)], cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.timeout)
        out = r.stdout.decode()
        sys.stdout.write(out)
        sys.stdout.flush()
        if r.returncode != 0:  # after a failed child nothing more is started on the device
            sys.stderr.write(r.stderr.decode()[-4000:])
            return r.returncode
        lines += [l for l in out.splitlines() if l.startswith("{")]
    if lines:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
