"""Times the batch inversion on the GPU (DESIGN_APPENDIX.md A.20; raw output: profiles/inverse/).

There is no earlier way to invert on the device, so the yardsticks are, per shape, in one child process per shape (each under its own
time limit):
  (new) sr_inverse_batch_dev, without and with numerators, through the library;
  (b)   sr_mul_elem_batch_dev on the same shape -- one read and one write of the table, the streaming bound -- alternating with (new);
  (a)   the same kernel at chunk 1, a Fermat inversion per unit, and at the neighbouring chunk lengths, alternating with the chosen
        chunk inside tools/ubench/inverse_bench.hip (built into build_tmp/ on first use): the library has no switch for it.
Device events sit around every timed piece; every contender is warmed up first.  Per contender the median and the spread
(max - min) / median are reported; `beats_chunk1` says whether the chosen chunk's median is below chunk 1's by more than the larger of
the two spreads.  Prints one JSON line per shape.

    python tools/bench_inverse.py [--reps 7] [--small] [--out FILE] [--timeout 400]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
UBENCH_SRC = os.path.join(ROOT, "tools", "ubench", "inverse_bench.hip")
UBENCH = os.path.join(ROOT, "build_tmp", "inverse_bench")

# (ring, log2 D, log2 n)
SHAPES = [("goldilocks", 16, 12), ("babybear", 16, 12), ("stark", 12, 12), ("goldilocks24", 0, 22), ("babybear72", 0, 20), ("frog16", 0, 22)]
SMALL = [("goldilocks", 16, 6), ("babybear", 16, 6), ("stark", 12, 6), ("goldilocks24", 0, 16), ("babybear72", 0, 14), ("frog16", 0, 16)]


def stat(xs):
    med = statistics.median(xs)
    return {"ms_median": round(med, 4), "ms_min": round(min(xs), 4), "ms_max": round(max(xs), 4), "spread": round((max(xs) - min(xs)) / med, 4)}


def build_ubench():
    if os.path.exists(UBENCH) and os.path.getmtime(UBENCH) >= os.path.getmtime(UBENCH_SRC):
        return
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(os.path.dirname(UBENCH), exist_ok=True)
    subprocess.check_call([hipcc if os.path.exists(hipcc) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-o", UBENCH, UBENCH_SRC], cwd=ROOT)


def run_shape(name, k, nv, reps):
    import torch

    from stark_rings_amd import CyclotomicRing, inverse_dev, inverse_plan, inverse_zero_count

    assert torch.cuda.is_available(), "bench_inverse needs a GPU"
    ring = CyclotomicRing(name, k, device=0)
    w = ring.words_per_elem
    eb, n = w * 8, 1 << nv
    new = lambda elems: torch.empty(elems * w, dtype=torch.int64, device="cuda")  # noqa: E731
    den, num, out, scratch = new(n), new(n), new(n), new(n)
    ring.fill_uniform_dev(den, 0xB000, 0)
    ring.fill_uniform_dev(num, 0xB001, 0)
    ring.fill_uniform_dev(scratch, 0xB002, 0)
    elem = num[:w].clone()
    pieces = {"inverse": lambda: inverse_dev(ring, out, den), "divide": lambda: inverse_dev(ring, out, den, num),
              "b_mul_elem": lambda: ring.mul_elem_dev(scratch, elem)}
    for f in pieces.values():
        f()
        f()
    torch.cuda.synchronize()
    zeros = inverse_zero_count(ring)   # uniform slots are zero with probability 1 / |F|: BabyBear's 2^28 coefficients hold a few
    ms = {key: [] for key in pieces}
    for _ in range(reps):
        for key, f in pieces.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[key].append(a.elapsed_time(b))
    res = {"ring": name, "log2_degree": k, "log2_n": nv, "table_bytes": n * eb, "reps": reps, "zero_slots_in_warmup": zeros,
           "chunk": inverse_plan(ring, n, False)[2], "chunk_num": inverse_plan(ring, n, True)[2]}
    for key in pieces:
        res[key] = stat(ms[key])
        traffic = (3 if key == "divide" else 2) * n * eb
        res[key]["tb_per_s"] = round(traffic / (res[key]["ms_median"] * 1e-3) / 1e12, 3)
    res["inverse_over_b"] = round(res["inverse"]["ms_median"] / res["b_mul_elem"]["ms_median"], 3)
    res["divide_over_b"] = round(res["divide"]["ms_median"] / res["b_mul_elem"]["ms_median"], 3)
    ring.close()
    del den, num, out, scratch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    # (a): the chunk lengths, in a process of its own that starts after this one has let go of its tables
    r = subprocess.run([UBENCH, name, str(k), str(nv), str(reps)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        sys.exit(r.returncode)
    u = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    res["chunks"] = {key: stat(v) for key, v in u["ms"].items()}
    for kind, c1 in (("chosen", "chunk1"), ("chosen_num", "chunk1_num")):
        a, b = res["chunks"][kind], res["chunks"][c1]
        margin = max(a["spread"], b["spread"])
        res[kind + "_over_chunk1"] = round(a["ms_median"] / b["ms_median"], 4)
        res[kind + "_beats_chunk1"] = bool(a["ms_median"] < b["ms_median"] * (1 - margin))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="tables 2^6 times smaller (a quick check of the tool itself)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=400, help="seconds one shape's child process may take")
    ap.add_argument("--shape", default=None, help="(internal) ring,log2_degree,log2_n: run this shape in this process")
    args = ap.parse_args()
    if args.shape:
        name, k, nv = args.shape.split(",")
        run_shape(name, int(k), int(nv), args.reps)
        return 0
    build_ubench()
    lines = []
    for name, k, nv in (SMALL if args.small else SHAPES):
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--shape", "%s,%d,%d" % (name, k, nv)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("bench_inverse: %s 2^%d x 2^%d ran past %d s; stopping" % (name, k, nv, args.timeout), file=sys.stderr)
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
