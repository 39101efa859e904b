"""Times the sparse-matrix calls on the GPU (DESIGN_APPENDIX.md A.11; raw output: profiles/spgemm/).

For each shape, in one process and alternating per repetition:
  (a) sr_spgemm_ntt_dev, the numeric phase of A B on a fixed structural pattern (the pattern is host arithmetic and is timed apart,
      on the host clock),
  (b) sr_gather_batch_dev moving the values of A into the order of A^T (the device part of a sparse transpose), and, where the dense
      operands fit,
  (c) what a caller had before for the same product: sr_matmul_ntt_dev on to_dense(A) and to_dense(B) (the densification is NOT counted).
(a) is reported as ring elements per second against the two traffic bounds of the appendix: nnz_a + nnz_b + n_out elements when every
operand element is fetched from memory once, 2 n_pairs + n_out when no fetch is reused.  (b) moves nnz_a elements in and nnz_a out.
Device events sit around every timed piece; every piece is first run for --ramp-ms so that code objects are loaded and the clocks
are up; to_dense of (a) is checked against (c) once.  Prints one JSON line per shape.

    python tools/bench_spgemm.py [--reps 20] [--small] [--out profiles/spgemm/bench_spgemm.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (ring, log2 D, n, m, p, stored entries per row of A, per row of B); the sizes of the large rings are those of tools/bench_next_rows.py
SHAPES = [("goldilocks", 10, 64, 1024, 64, 64, 8), ("goldilocks", 16, 32, 64, 32, 16, 8), ("babybear", 16, 32, 64, 32, 16, 8),
          ("stark", 12, 32, 128, 32, 32, 8), ("goldilocks24", 0, 512, 2048, 512, 64, 16), ("babybear72", 0, 512, 2048, 512, 64, 16),
          ("frog16", 0, 512, 2048, 512, 64, 16)]
SHAPES_SMALL = [("goldilocks", 10, 8, 32, 8, 8, 4), ("goldilocks", 16, 2, 4, 2, 2, 2), ("babybear", 16, 2, 4, 2, 2, 2), ("stark", 12, 4, 8, 4, 4, 2),
                ("goldilocks24", 0, 16, 64, 16, 8, 4), ("babybear72", 0, 16, 64, 16, 8, 4), ("frog16", 0, 16, 64, 16, 8, 4)]
DENSE_LIMIT_BYTES = 8 << 30  # to_dense(A), to_dense(B) and the dense product together


def pattern(rng, nrows, ncols, per_row):
    """per_row distinct columns in every row, ascending"""
    cols = np.concatenate([np.sort(rng.choice(ncols, per_row, replace=False)) for _ in range(nrows)]).astype(np.uint32)
    return cols, np.arange(0, nrows * per_row + 1, per_row, dtype=np.uint64)


def timed(torch, pieces, reps, ramp_ms):
    for f in pieces.values():
        t0 = time.perf_counter()
        while True:
            f()
            torch.cuda.synchronize()
            if (time.perf_counter() - t0) * 1e3 >= ramp_ms:
                break
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
    ap.add_argument("--ramp-ms", type=float, default=200.0)
    ap.add_argument("--small", action="store_true", help="small shapes (a quick check of the tool itself)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spgemm", "bench_spgemm.jsonl"))
    args = ap.parse_args()
    import torch

    from stark_rings_amd import CyclotomicRing, SparseMatrixNTT
    from stark_rings_amd.rings import sparse_transpose_pattern, spgemm_pattern

    assert torch.cuda.is_available(), "bench_spgemm needs a GPU"
    results = []
    new = lambda n, t=torch.int64: torch.empty(n, dtype=t, device="cuda")  # noqa: E731
    for name, k, n, m, p, row_a, row_b in (SHAPES_SMALL if args.small else SHAPES):
        ring = CyclotomicRing(name, k, device=0)
        w = ring.words_per_elem
        rng = np.random.default_rng(1000 * k + n)
        a_cols, a_ptr = pattern(rng, n, m, row_a)
        b_cols, b_ptr = pattern(rng, m, p, row_b)
        t0 = time.perf_counter()
        out_ptr, out_cols, pair_ptr, pair_a, pair_b = spgemm_pattern(a_cols, a_ptr, n, m, b_cols, b_ptr, p)
        pattern_ms = (time.perf_counter() - t0) * 1e3
        _, _, perm = sparse_transpose_pattern(a_cols, a_ptr, n, m)
        nnz_a, nnz_b, n_out, n_pairs = a_cols.size, b_cols.size, out_cols.size, pair_a.size
        a_vals, b_vals = new(nnz_a * w), new(nnz_b * w)
        ring.fill_uniform_dev(a_vals, 0x5B11 + n, 0)
        ring.fill_uniform_dev(b_vals, 0x5B12 + n, 0)
        out, live, moved = new(n_out * w), new(n_out, torch.int32), new(nnz_a * w)
        d_ptr, d_pa, d_pb, d_perm = (torch.from_numpy(x.view(t)).cuda() for x, t in ((pair_ptr, np.int64), (pair_a, np.int32), (pair_b, np.int32),
                                                                                      (perm, np.int32)))
        pieces = {"a_spgemm": lambda: ring.spgemm_ntt_dev(out, live, a_vals, b_vals, d_ptr, d_pa, d_pb),
                  "b_gather": lambda: ring.gather_dev(moved, a_vals, d_perm)}
        elem_bytes = w * 8
        dense_fits = (n * m + m * p + n * p) * elem_bytes <= DENSE_LIMIT_BYTES
        if dense_fits:
            da = SparseMatrixNTT(ring, n, m, a_vals, a_cols, a_ptr).to_dense()
            db = SparseMatrixNTT(ring, m, p, b_vals, b_cols, b_ptr).to_dense()
            full = new(n * p * w)
            pieces["c_matmul_dense"] = lambda: ring.matmul_ntt_dev(full, da, db, n, m, p)
        t = timed(torch, pieces, args.reps, args.ramp_ms)
        dead = ring.spgemm_dead_count()
        assert ring.spmv_bad_index_count() == 0
        sec = t["a_spgemm"]["ms_median"] * 1e-3
        lower, upper = nnz_a + nnz_b + n_out, 2 * n_pairs + n_out
        res = {"ring": name, "log2_degree": k, "n": n, "m": m, "p": p, "nnz_a": nnz_a, "nnz_b": nnz_b, "n_out": n_out, "n_pairs": n_pairs,
               "elem_bytes": elem_bytes, "reps": args.reps, "dead_entries_per_call": dead // max(1, args.reps), "pattern_host_ms": round(pattern_ms, 3), **t,
               "spgemm_elems_per_s_lower_bound_traffic": round(lower / sec), "spgemm_elems_per_s_no_reuse_traffic": round(upper / sec),
               "spgemm_gb_per_s_lower_bound_traffic": round(lower * elem_bytes / sec / 1e9, 1),
               "spgemm_gb_per_s_no_reuse_traffic": round(upper * elem_bytes / sec / 1e9, 1),
               "slot_macs_per_s": round(n_pairs * ring.degree / sec),
               "gather_elems_per_s_load_plus_store": round(2 * nnz_a / (t["b_gather"]["ms_median"] * 1e-3)),
               "gather_gb_per_s_load_plus_store": round(2 * nnz_a * elem_bytes / (t["b_gather"]["ms_median"] * 1e-3) / 1e9, 1)}
        if dense_fits:
            got = SparseMatrixNTT(ring, n, p, out, out_cols, out_ptr).to_dense()
            res["to_dense_equals_matmul"] = bool(torch.equal(got, full))
            res["spgemm_over_dense_matmul_time"] = round(t["a_spgemm"]["ms_median"] / t["c_matmul_dense"]["ms_median"], 4)
            res["matmul_spread"] = round((t["c_matmul_dense"]["ms_max"] - t["c_matmul_dense"]["ms_min"]) / t["c_matmul_dense"]["ms_median"], 3)
            del da, db, full, got
        print(json.dumps(res), flush=True)
        results.append(res)
        ring.close()
        del a_vals, b_vals, out, live, moved, pieces
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for res in results:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
