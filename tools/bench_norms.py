"""Times the norm kernels on the GPU beside two passes that existed before them (DESIGN_APPENDIX.md A.6; raw output: profiles/norms/).

For each buffer, in one process and alternating per repetition:
  (y1) evaluate through sr_mle_fix_variables_dev (power-of-two element counts only): the library's best read-once pass;
  (y2) sr_count_noncanonical_dev: a read-only pass with one atomic per lane (it synchronises: timed with the same events);
  (n*) sr_norm_batch_dev for which = 1, 2, 3 over the whole slice and per ring element.
Device events sit around every timed piece; every shape is warmed up first.  The yardsticks' own spread (max - min over the repeats,
relative to the median) is printed so that "within the spread" can be read off.  Prints one JSON line per buffer.

    python tools/bench_norms.py [--reps 10] [--small] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# ring, log2 D, log2 of the element count: Goldilocks and BabyBear 8 GiB, Stark 512 MiB, goldilocks24 x 2^24 (3 GiB)
BUFFERS = [("goldilocks", 16, 14), ("babybear", 16, 14), ("stark", 12, 12), ("goldilocks24", 0, 24)]
SMALL = [("goldilocks", 16, 8), ("babybear", 16, 8), ("stark", 12, 6), ("goldilocks24", 0, 18)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="buffers 2^6 times smaller (a quick check of the tool itself)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from stark_rings_amd import CyclotomicRing

    assert torch.cuda.is_available(), "bench_norms needs a GPU"
    results = []
    for name, k, nv in (SMALL if args.small else BUFFERS):
        ring = CyclotomicRing(name, k, device=0)
        w = ring.words_per_elem
        n_elems = 1 << nv
        n_coeffs = n_elems * ring.degree
        nbytes = n_elems * w * 8
        data = torch.empty(n_elems * w, dtype=torch.int64, device="cuda")
        ring.fill_uniform_dev(data, 0xB0B, 0)
        point = torch.empty(nv * w, dtype=torch.int64, device="cuda")
        ring.fill_uniform_dev(point, 0xB0C, 0)
        mle_work = torch.empty(max(ring.mle_plan(nv, nv)[0], 1) * w, dtype=torch.int64, device="cuda")
        mle_out = torch.empty(w, dtype=torch.int64, device="cuda")
        pieces = {"y1_mle_evaluate": lambda: ring.mle_fix_variables_dev(mle_out, data, nv, point, 0, mle_work),
                  "y2_count_noncanonical": lambda: ring.count_noncanonical_dev(data)}
        plans = {}
        for which in (1, 2, 3):
            for label, group in (("slice", n_coeffs), ("per_elem", ring.degree)):
                wpg, need, launches = ring.norm_plan(n_coeffs, group, which)
                out = torch.empty(n_coeffs // group * wpg, dtype=torch.int64, device="cuda")
                work = torch.empty(max(need, 1), dtype=torch.int64, device="cuda")
                key = "n%d_%s" % (which, label)
                plans[key] = {"launches": launches, "work_words": need}
                pieces[key] = (lambda o=out, g=group, wh=which, wk=work: ring.norm_batch_dev(o, data, g, wh, wk))
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
        res = {"ring": name, "log2_degree": k, "log2_elems": nv, "bytes": nbytes, "reps": args.reps}
        for key in pieces:
            med = statistics.median(ms[key])
            res[key] = {"ms_median": round(med, 4), "ms_min": round(min(ms[key]), 4), "ms_max": round(max(ms[key]), 4),
                        "spread": round((max(ms[key]) - min(ms[key])) / med, 3), "tb_per_s": round(nbytes / (med * 1e-3) / 1e12, 3)}
            if key in plans:
                res[key].update(plans[key])
                res[key]["over_y1"] = round(med / statistics.median(ms["y1_mle_evaluate"]), 3)
                res[key]["over_y2"] = round(med / statistics.median(ms["y2_count_noncanonical"]), 3)
        print(json.dumps(res), flush=True)
        results.append(res)
        ring.close()
        del data, mle_work, pieces
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for res in results:
                f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
