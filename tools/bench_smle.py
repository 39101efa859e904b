"""Times the sparse multilinear-extension calls on the GPU (DESIGN_APPENDIX.md A.7; raw output: profiles/smle/).

For each shape, in one process and alternating per repetition, each row next to a yardstick from entry points that existed before:
  (a) evaluate (n_fixed = num_vars) of nnz stored entries by the plan sr_smle_plan chooses, against
  (b) sr_mul_elem_add_batch_dev over a batch of nnz elements (moves 3 nnz elements where the fold moves about nnz plus cached gathers);
  (c) sr_eq_table_dev of n_eq variables, against
  (d) sr_mle_fix_variables_dev with n_fixed = 0 of the same number of elements (a copy: the store stream alone);
  (e) the fold with every run one entry (n_fixed small, n_out = nnz): the one-launch shape.
Device events sit around every timed piece; every shape is warmed up first.  Prints one JSON line per shape.

    python tools/bench_smle.py [--reps 20] [--small] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (ring, log2 D, log2 nnz, num_vars = n_fixed of the evaluate, n_eq)
SHAPES = [("goldilocks", 10, 20, 40, 18), ("goldilocks24", 0, 24, 40, 24), ("stark", 12, 12, 40, 10), ("babybear", 10, 20, 40, 18)]
SMALL = [("goldilocks", 10, 14, 40, 12), ("goldilocks24", 0, 18, 40, 18), ("stark", 12, 8, 40, 6), ("babybear", 10, 14, 40, 12)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="shapes 2^6 times smaller (a quick check of the tool itself)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from stark_rings_amd import CyclotomicRing
    from stark_rings_amd.rings import MLE_LEADING, smle_fix_pattern

    assert torch.cuda.is_available(), "bench_smle needs a GPU"
    results = []
    for name, k, lognnz, nv, n_eq in (SMALL if args.small else SHAPES):
        ring = CyclotomicRing(name, k, device=0)
        w = ring.words_per_elem
        eb = w * 8
        nnz = 1 << lognnz
        rng = np.random.default_rng(0x5B1E + lognnz)
        idx = np.unique(rng.integers(0, 1 << nv, size=nnz + nnz // 8, dtype=np.uint64))[:nnz]
        assert idx.size == nnz
        new = lambda n: torch.empty(n * w, dtype=torch.int64, device="cuda")
        vals, acc, point = new(nnz), new(nnz), new(nv)
        for t, seed in ((vals, 1), (acc, 2), (point, 3)):
            ring.fill_uniform_dev(t, 0xBE90 + seed, 0)
        d_idx = torch.from_numpy(idx.view(np.int64)).cuda()
        shapes = {}
        for key, nf in (("evaluate", nv), ("singletons", 1)):
            keys, seg = smle_fix_pattern(idx, nv, nf)
            work_elems, launches = ring.smle_plan(nnz, keys.size, nf)
            shapes[key] = (nf, keys.size, torch.from_numpy(seg.view(np.int64)).cuda(), new(max(work_elems, 1)), new(keys.size), work_elems, launches)
        eq_out, copy_out = new(1 << n_eq), new(1 << n_eq)

        def fold(key):
            nf, n_out, d_seg, work, out, work_elems, _ = shapes[key]
            ring.smle_fix_variables_dev(out, vals, d_idx, d_seg, point[:nf * w], work if work_elems else None)

        pieces = {
            "a_evaluate": lambda: fold("evaluate"),
            "b_mul_elem_add": lambda: ring.mul_elem_add_dev(acc, vals, point[:w]),
            "c_eq_table": lambda: ring.eq_table_dev(eq_out, point[:n_eq * w]),
            "d_copy": lambda: ring.mle_fix_variables_dev(copy_out, eq_out, n_eq, None, MLE_LEADING, None),
            "e_singletons": lambda: fold("singletons"),
        }
        nbytes = {"a_evaluate": nnz * (eb + 8), "b_mul_elem_add": 3 * nnz * eb, "c_eq_table": eb << n_eq, "d_copy": 2 * (eb << n_eq),
                  "e_singletons": nnz * (eb + 8) + shapes["singletons"][1] * eb}
        for f in pieces.values():
            f()
            f()
        torch.cuda.synchronize()
        ms = {key: [] for key in pieces}
        for _ in range(args.reps):
            for key, f in pieces.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                ms[key].append(a.elapsed_time(b))
        res = {"ring": name, "log2_degree": k, "nnz": nnz, "num_vars": nv, "n_eq": n_eq, "reps": args.reps,
               "evaluate_launches": shapes["evaluate"][6], "evaluate_work_elems": shapes["evaluate"][5],
               "singletons_launches": shapes["singletons"][6], "singletons_n_out": shapes["singletons"][1]}
        for key in pieces:
            med = statistics.median(ms[key])
            res[key] = {"ms_median": round(med, 4), "ms_min": round(min(ms[key]), 4), "ms_max": round(max(ms[key]), 4), "bytes": nbytes[key],
                        "tb_per_s": round(nbytes[key] / (med * 1e-3) / 1e12, 3)}
        res["evaluate_over_yardstick_time"] = round(res["a_evaluate"]["ms_median"] / res["b_mul_elem_add"]["ms_median"], 3)
        res["yardstick_spread"] = round((res["b_mul_elem_add"]["ms_max"] - res["b_mul_elem_add"]["ms_min"]) / res["b_mul_elem_add"]["ms_median"], 3)
        res["eq_table_over_copy_time"] = round(res["c_eq_table"]["ms_median"] / res["d_copy"]["ms_median"], 3)
        print(json.dumps(res), flush=True)
        results.append(res)
        ring.close()
        del vals, acc, eq_out, copy_out, shapes
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for res in results:
                f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
