"""INTEGRATION.md section 3 is a patch against the reference crate that must not add a second impl of a trait a type already has
(error E0119; stable Rust has no specialisation).  No Rust toolchain exists in this image, so the check is by reading -- and this test
makes the reading reproducible: every reference line the recipe says it replaces or edits is where the recipe says it is, and the
traits it hooks have exactly the impls the recipe lists.  The reference is read through tests/golden/reference_recipe_index.json
(line hashes and impl query hits, no source text; regenerated from a reference checkout by tests/golden/make_recipe_index.py)."""
import hashlib
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEX = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_recipe_index.json")))
LINES = {(e["file"], e["line"]): e["sha256"] for e in INDEX["lines"]}


def _line_is(rel, n, text):
    """line n of rel, stripped, is exactly `text`"""
    return LINES[(rel, n)] == hashlib.sha256(text.strip().encode()).hexdigest()


def _grep(name, pattern):
    q = INDEX["impls"][name]
    assert q["pattern"] == pattern, (name, q["pattern"])   # the index answers the question asked here
    return [tuple(h) for h in q["hits"]]


def test_the_lines_the_recipe_replaces_are_where_it_says():
    # the four macro invocations the patch puts behind #[cfg(not(feature = "hip"))]
    for rel, n, cfg in (("cyclotomic_ring/models/goldilocks/mod.rs", 151, "GoldilocksRingConfig"),
                        ("cyclotomic_ring/models/babybear/mod.rs", 163, "BabyBearRingConfig"),
                        ("cyclotomic_ring/models/stark_prime/mod.rs", 97, "StarkRingConfig"),
                        ("cyclotomic_ring/models/frog_ring/mod.rs", 135, "FrogRingConfig")):
        assert _line_is(rel, n, "impl_crt_icrt_for_a_ring!(RqNTT, RqPoly, %s);" % cfg), (rel, n)
    # the impl blocks it edits in place
    assert _line_is("cyclotomic_ring/models/goldilocks/mod.rs", 69, "impl CyclotomicConfig<1> for GoldilocksRingConfig {")
    assert _line_is("cyclotomic_ring/models/babybear/mod.rs", 81, "impl CyclotomicConfig<1> for BabyBearRingConfig {")
    assert _line_is("cyclotomic_ring/models/frog_ring/mod.rs", 72, "impl CyclotomicConfig<1> for FrogRingConfig {")
    assert _line_is("cyclotomic_ring/models/stark_prime/mod.rs", 34, "impl CyclotomicConfig<4> for StarkRingConfig {")
    assert _line_is("cyclotomic_ring/coeff_form.rs", 588, "impl<C: CyclotomicConfig<N>, const N: usize, const D: usize> Decompose")
    assert _line_is("cyclotomic_ring/coeff_form.rs", 589, "for CyclotomicPolyRingGeneral<C, N, D>")
    assert _line_is("balanced_decomposition/mod.rs", 21, "pub trait Decompose: Ring {")
    assert _line_is("balanced_decomposition/mod.rs", 163, "impl<R: Decompose> GadgetDecompose for &[R] {")
    assert _line_is("cyclotomic_ring/ring_config.rs", 11, "pub trait CyclotomicConfig<const N: usize>: Send + Sync + 'static + Sized {")
    assert _line_is("cyclotomic_ring/crt.rs", 10, "fn elementwise_crt(vec: Vec<Self>) -> Vec<Self::CRTForm> {")
    assert _line_is("cyclotomic_ring/crt.rs", 34, "fn elementwise_icrt(vec: Vec<Self>) -> Vec<Self::ICRTForm> {")


def test_no_trait_the_recipe_touches_has_an_impl_it_would_collide_with():
    # CRT / ICRT: implemented ONLY inside the macro (crt.rs) -- replacing the macro's expansion leaves exactly one impl per type
    crt = _grep("crt_icrt", r"impl\b.*\bI?CRT for\b")
    assert crt and all(rel == "cyclotomic_ring/crt.rs" for rel, _ in crt), crt
    # Decompose: the blanket impl for ConvertibleRing and the generic one for the coefficient-form ring; nothing per model
    dec = _grep("decompose", r"impl\b(?!.*Gadget).*[^a-zA-Z]Decompose\s*(for\b|$)")
    assert sorted(dec) == [("balanced_decomposition/convertible_ring.rs", 43), ("cyclotomic_ring/coeff_form.rs", 588)], dec
    # GadgetDecompose: blanket impls only (the recipe adds a call inside the one for &[R], no new impl)
    gd = _grep("gadget_decompose", r"impl<R: Decompose> GadgetDecompose for")
    assert sorted(n for rel, n in gd if rel == "balanced_decomposition/mod.rs") == [163, 192, 208, 276, 311]
    # CyclotomicConfig: four model impls, all edited in place
    cc = [rel for rel, _ in _grep("cyclotomic_config", r"^impl CyclotomicConfig<")]
    assert sorted(cc) == sorted("cyclotomic_ring/models/%s/mod.rs" % m for m in ("goldilocks", "babybear", "stark_prime", "frog_ring"))


def test_the_recipe_itself_declares_no_impl_of_an_existing_trait_for_an_existing_type():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("## 3. The patch"):text.index("## 4. Linking")]
    added = [ln[1:].strip() for ln in sec.split("\n") if ln.startswith("+") and not ln.startswith("+++")]
    heads = [ln for ln in added if re.match(r"impl\b", ln)]
    # the only impl headers on '+' lines are the two inside the replacement macro (generic over $icrt / $crt)
    assert heads == ["impl CRT for $icrt {", "impl ICRT for $crt {"], heads
    # outside the diff, the one new impl is for a NEW type
    rust_blocks = re.findall(r"```rust\n(.*?)```", sec, flags=re.S)   # (context lines of the ```diff blocks are the reference's own text)
    free = [ln.strip() for blk in rust_blocks for ln in blk.split("\n") if re.match(r"\s*impl\b", ln)]
    assert free and all("GoldilocksPow2Config" in ln for ln in free), free
