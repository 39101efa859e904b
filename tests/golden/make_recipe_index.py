#!/usr/bin/env python3
"""Index of the reference crate for tests/test_integration_recipe.py: where the lines INTEGRATION.md section 3 edits are, and where
the impls of the traits it hooks are.

    python tests/golden/make_recipe_index.py <reference checkout>      (or SR_REFERENCE=<reference checkout>)

writes tests/golden/reference_recipe_index.json.  The output is DATA: for every cited line its file, line number and the sha256 of
its text with surrounding whitespace stripped, and for every impl query its regular expression and the (file, line) of each hit.
No reference source text is kept, so the test checks the recipe against this index without the reference tree."""
import hashlib
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_recipe_index.json")
CRATE = "crates/ring/src"

# the lines the recipe replaces (the four macro invocations) or edits in place, and the trait / method heads it relies on
CITED = [
    ("cyclotomic_ring/models/goldilocks/mod.rs", 151), ("cyclotomic_ring/models/babybear/mod.rs", 163),
    ("cyclotomic_ring/models/stark_prime/mod.rs", 97), ("cyclotomic_ring/models/frog_ring/mod.rs", 135),
    ("cyclotomic_ring/models/goldilocks/mod.rs", 69), ("cyclotomic_ring/models/babybear/mod.rs", 81),
    ("cyclotomic_ring/models/frog_ring/mod.rs", 72), ("cyclotomic_ring/models/stark_prime/mod.rs", 34),
    ("cyclotomic_ring/coeff_form.rs", 588), ("cyclotomic_ring/coeff_form.rs", 589),
    ("balanced_decomposition/mod.rs", 21), ("balanced_decomposition/mod.rs", 163),
    ("cyclotomic_ring/ring_config.rs", 11), ("cyclotomic_ring/crt.rs", 10), ("cyclotomic_ring/crt.rs", 34),
]

# every impl of a trait the recipe touches (one line per hit; a Gadget* impl is not a Decompose impl)
QUERIES = {
    "crt_icrt": r"impl\b.*\bI?CRT for\b",
    "decompose": r"impl\b(?!.*Gadget).*[^a-zA-Z]Decompose\s*(for\b|$)",
    "gadget_decompose": r"impl<R: Decompose> GadgetDecompose for",
    "cyclotomic_config": r"^impl CyclotomicConfig<",
}


def sha(text):
    return hashlib.sha256(text.strip().encode()).hexdigest()


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SR_REFERENCE")
    if not ref:
        raise SystemExit(__doc__)
    src = os.path.join(ref, CRATE)
    files = {}
    for d, _, names in os.walk(src):
        for f in names:
            if f.endswith(".rs"):
                p = os.path.join(d, f)
                files[os.path.relpath(p, src)] = open(p).read().split("\n")
    lines = [{"file": rel, "line": n, "sha256": sha(files[rel][n - 1])} for rel, n in CITED]
    impls = {}
    for name, pattern in QUERIES.items():
        hits = [[rel, i] for rel in sorted(files) for i, ln in enumerate(files[rel], 1) if re.search(pattern, ln)]
        impls[name] = {"pattern": pattern, "hits": hits}
    out = {"_about": "locations in the reference crate (%s) that INTEGRATION.md section 3 relies on: line hashes and impl query hits; "
                     "no source text (tests/golden/make_recipe_index.py)" % CRATE,
           "lines": lines, "impls": impls}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
