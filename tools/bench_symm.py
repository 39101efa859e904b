"""Times the symmetric-matrix calls on the GPU (DESIGN_APPENDIX.md A.8; raw output: profiles/symm/).

For each Gram shape, in one process and alternating per repetition:
  (a) sr_gram_ntt_dev by the plan sr_gram_plan chooses, against
  (b) what the library offered before for the same result: sr_matmul_ntt_dev(A, A^T) with A^T already on the device (the host
      transposition and the repacking into the lower triangle are NOT counted).
For each recompose shape: sr_symm_recompose_dev, reported as bytes of `mat` per second, next to
  (c) sr_mle_fix_variables_dev with n_fixed = 0 over the same number of elements (a copy: one load and one store stream).
Device events sit around every timed piece; every shape is warmed up first; the result of (a) is checked against (b) once.
Prints one JSON line per shape.

    python tools/bench_symm.py [--reps 20] [--small] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (ring, log2 D, n, m)
GRAM = [("goldilocks24", 0, 64, 4096), ("goldilocks24", 0, 8, 65536), ("babybear72", 0, 64, 4096), ("babybear72", 0, 8, 65536),
        ("goldilocks", 10, 64, 256)]
GRAM_SMALL = [("goldilocks24", 0, 16, 256), ("goldilocks24", 0, 4, 1024), ("babybear72", 0, 16, 256), ("babybear72", 0, 4, 1024),
              ("goldilocks", 10, 16, 16)]
# (ring, log2 D, n, d): mat holds (n d)(n d + 1) / 2 elements
RECOMPOSE = [("goldilocks", 10, 256, 4), ("babybear", 10, 256, 4), ("stark", 8, 128, 4), ("goldilocks24", 0, 1024, 4), ("babybear72", 0, 512, 4)]
RECOMPOSE_SMALL = [("goldilocks", 10, 16, 4), ("babybear", 10, 16, 4), ("stark", 8, 8, 4), ("goldilocks24", 0, 64, 4), ("babybear72", 0, 32, 4)]


def timed(torch, pieces, reps):
    for f in pieces.values():
        f()
        f()
    torch.cuda.synchronize()
    ms = {key: [] for key in pieces}
    for _ in range(reps):
        for key, f in pieces.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[key].append(a.elapsed_time(b))
    return {key: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for key, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="small shapes (a quick check of the tool itself)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from stark_rings_amd import CyclotomicRing
    from stark_rings_amd.rings import MLE_LEADING

    assert torch.cuda.is_available(), "bench_symm needs a GPU"
    results = []
    new = lambda n: torch.empty(n, dtype=torch.int64, device="cuda")  # noqa: E731
    for name, k, n, m in (GRAM_SMALL if args.small else GRAM):
        ring = CyclotomicRing(name, k, device=0)
        w = ring.words_per_elem
        packed = n * (n + 1) // 2
        a = new(n * m * w)
        ring.fill_uniform_dev(a, 0x5A11 + n, 0)
        at = a.view(n, m, w).transpose(0, 1).contiguous().view(-1)
        work_elems, launches = ring.gram_plan(n, m)
        work = new(work_elems * w) if work_elems else None
        out, full = new(packed * w), new(n * n * w)
        pieces = {"a_gram": lambda: ring.gram_ntt_dev(out, a, n, m, work), "b_matmul_a_at": lambda: ring.matmul_ntt_dev(full, a, at, n, m, n)}
        t = timed(torch, pieces, args.reps)
        tri = torch.tril_indices(n, n)
        same = bool(torch.equal(out.view(packed, w), full.view(n, n, w)[tri[0].cuda(), tri[1].cuda()]))
        res = {"call": "gram", "ring": name, "log2_degree": k, "n": n, "m": m, "reps": args.reps, "launches": launches, "work_elems": work_elems,
               "equals_lower_triangle_of_matmul": same, **t,
               "gram_over_matmul_time": round(t["a_gram"]["ms_median"] / t["b_matmul_a_at"]["ms_median"], 3),
               "matmul_spread": round((t["b_matmul_a_at"]["ms_max"] - t["b_matmul_a_at"]["ms_min"]) / t["b_matmul_a_at"]["ms_median"], 3)}
        print(json.dumps(res), flush=True)
        results.append(res)
        ring.close()
        del a, at, out, full, work
        torch.cuda.empty_cache()
    for name, k, n, d in (RECOMPOSE_SMALL if args.small else RECOMPOSE):
        ring = CyclotomicRing(name, k, device=0)
        w = ring.words_per_elem
        nd = n * d
        elems = nd * (nd + 1) // 2
        mat, powers = new(elems * w), new(d * w)
        ring.fill_uniform_dev(mat, 0x5A21 + n, 0)
        ring.fill_uniform_dev(powers, 0x5A22 + n, 0)
        out, work = new(n * (n + 1) // 2 * w), new(d * d * w)
        nv = max((elems - 1).bit_length(), 0)
        copy_out = new(w << nv)
        pieces = {"a_recompose": lambda: ring.symm_recompose_dev(out, mat, n, d, powers, work),
                  "c_copy": lambda: ring.mle_fix_variables_dev(copy_out, mat, nv, None, MLE_LEADING, None)}
        t = timed(torch, pieces, args.reps)
        mat_bytes = elems * w * 8
        res = {"call": "recompose", "ring": name, "log2_degree": k, "n": n, "d": d, "reps": args.reps, "mat_bytes": mat_bytes, **t,
               "mat_tb_per_s": round(mat_bytes / (t["a_recompose"]["ms_median"] * 1e-3) / 1e12, 3),
               "copy_tb_per_s_load_plus_store": round((mat_bytes + (w << nv) * 8) / (t["c_copy"]["ms_median"] * 1e-3) / 1e12, 3)}
        print(json.dumps(res), flush=True)
        results.append(res)
        ring.close()
        del mat, out, copy_out
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for res in results:
                f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
