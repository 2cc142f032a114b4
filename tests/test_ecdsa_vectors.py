"""Constructed ECDSA edge-case vectors (tests/ecdsa_vectors.py, docs/ECDSA_VECTORS.md) through the
CPU verifier and every GPU path of csrc/kernels/secp256k1.hip.

The expected verdicts come from the constructions and the pure-Python oracle
(bitcoincashplus_amd/utils/secp256k1_ref.py), never from the code under test. Families:
A: x(R) >= n and the r + n < p boundary; B: chosen u1 and u2 (comb windows, GLV halves);
C: chosen s; D: keys related to G (doubling and infinity in the additions); E: key encodings.

Dispatch of the two GPU entry points (csrc/kernels/secp256k1.hip):
  * native.ecdsa_verify_batch(use_gpu=True) -> GpuVerifyDeferred -> GpuVerifyService::EcdsaDerFill
    -> VerifyLane::EcdsaDerFill -> LaneEcdsa -> LaunchVerify(der = true): the device parses the DER
    bytes; PrepDerAndKey sends 33-byte keys with prefix 02 / 03 unparsed and parses the others on
    the host.
  * native.gpu_verify_ecdsa_packed (the bytes path of ops.ecdsa_verify_compact) ->
    GpuVerifyService::Ecdsa -> VerifyLane::Ecdsa -> EcdsaFill -> LaneEcdsa -> LaunchVerify(der =
    false): compact r || s, low s only, the 33 key bytes as they are (the device checks the prefix).
Both reach the same LaunchVerify, which reads both pins of test_ecdsa_batch.pin_path (the fused
maximum and the split kernel), so each entry point is run on all four paths. (EcdsaVerifyBatch and
EcdsaVerifyDevice, the tensor path, call the same LaunchVerify(der = false).)
"""
import pytest

import ecdsa_vectors as ev
from test_ecdsa_batch import PATHS, make_items, pin_path, unpin_path


@pytest.fixture(scope="module")
def vectors():
    return ev.build()


def _check(what, labels, got, expect):
    """Fails with one line per vector whose verdict is not the expected one."""
    assert len(got) == len(expect) == len(labels)
    bad = [f"  {labels[i]}: got {bool(got[i])}, expected {expect[i]}" for i in range(len(expect)) if bool(got[i]) != expect[i]]
    if bad:
        pytest.fail(f"{what}: {len(bad)} of {len(expect)} verdicts differ\n" + "\n".join(bad[:80]), pytrace=False)


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("family", sorted(ev.MIN_COUNTS))
def test_cpu_family(native, vectors, family):
    vs = vectors.family(family)
    res, _ = native.ecdsa_verify_batch([(v.pub, v.sig, v.msg) for v in vs], use_gpu=False)
    _check(f"CPU, family {family}", [v.label for v in vs], res, [v.expect for v in vs])


def test_vector_counts(vectors):
    """Every family has at least its stated number of vectors, every vector belongs to a family,
    and nothing was dropped but high-s retries: each call of the builder's add() is a vector, and
    family D's doubling and equal-halves vectors (fixed key and scalars: a candidate with a high s
    is left out, it cannot be drawn again) are counted."""
    print(f"{len(vectors.vectors)} vectors built in {vectors.seconds:.1f} s, {vectors.retries} high-s retries")
    assert len(vectors.vectors) == vectors.oracle_calls
    assert sum(len(vectors.family(f)) for f in ev.MIN_COUNTS) == len(vectors.vectors)
    for f, least in ev.MIN_COUNTS.items():
        assert len(vectors.family(f)) >= least, f
    doubling = [v for v in vectors.vectors if v.label.startswith("D.double.")]
    assert len(doubling) == vectors.kept_doubling >= 3
    equal = [v for v in vectors.vectors if v.label.startswith("D.equal_halves.")]
    assert len(equal) == vectors.kept_equal_halves >= 3
    assert len([v for v in vectors.vectors if v.label.startswith("D.opposite_halves.")]) == len(equal)
    left_out = len(ev.DOUBLING_CANDIDATES) - len(doubling) + len(ev.EQUAL_HALVES_CANDIDATES) - len(equal)
    assert vectors.retries >= left_out
    # both verdicts in the families that have both, and enough for the compact entry point
    for f in "ADE":
        assert {v.expect for v in vectors.family(f)} == {True, False}
    twins = [c for c in vectors.compact if c[0].startswith("C.twin.")]
    assert len(twins) >= 3 and not any(c[4] for c in twins)
    assert len(vectors.compact) >= 200


# ------------------------------------------------------------------ GPU
def _arrange(native, vectors, how):
    """(labels, items, expected) of one batch. Every batch ends with an edge vector (the fused and
    the half-lane kernel recompute the last signature in the lanes past the end) and its length is
    no multiple of 64.
      in_order:    the vectors as built.
      reversed:    ordinary signatures in front so that every vector lands in the other half of a
                   64-lane block than in_order (asserted), then the vectors backwards.
      interleaved: vector, ordinary, vector, ...: every vector between lanes doing ordinary work.
    """
    vs = list(vectors.vectors)
    n = len(vs)
    plain_items, plain_expect = make_items(native, n + 64, seed=29)
    plain = [(f"ordinary.{i}", it, ok) for i, (it, ok) in enumerate(zip(plain_items, plain_expect))]
    edge = [(v.label, (v.pub, v.sig, v.msg), v.expect) for v in vs]
    if how == "in_order":
        batch = edge + ([edge[0]] if n % 64 == 0 else [])
    elif how == "reversed":
        front = (-n) % 64  # vector i sits at front + n - 1 - i = 63 - i (mod 64)
        batch = plain[:front] + edge[::-1] + [edge[0]]
        for i in range(n):
            assert batch[front + n - 1 - i][0] == edge[i][0]
            assert ((front + n - 1 - i) % 64 < 32) != (i % 64 < 32)
    elif how == "interleaved":
        batch = [x for pair in zip(edge, plain) for x in pair][:-1]
    else:
        raise ValueError(how)
    assert len(batch) % 64 != 0 and not batch[-1][0].startswith("ordinary")
    return [b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch]


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["in_order", "reversed", "interleaved"])
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_der_vectors(native, vectors, path, how):
    """The full set through native.ecdsa_verify_batch(use_gpu=True) (device DER parse) on one
    pinned path, in one arrangement."""
    labels, items, expect = _arrange(native, vectors, how)
    old = pin_path(native, path)
    try:
        got, _ = native.ecdsa_verify_batch(items, use_gpu=True)
    finally:
        unpin_path(native, old)
    _check(f"{path}, {how}", labels, got, expect)


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_compact_vectors(native, vectors, path):
    """The compressed-key, low-s vectors and family C's high-s twins (invalid here) through the
    compact entry point native.gpu_verify_ecdsa_packed, which obeys both pins (module docstring):
    as built, and backwards behind as many ordinary signatures as put every vector into the other
    half of a 64-lane block (asserted)."""
    comp = list(vectors.compact)
    n = len(comp)
    plain_items, plain_expect = make_items(native, 4 * 96, seed=31)
    plain = []
    for (pub, sig, msg), ok in zip(plain_items, plain_expect):
        if len(pub) != 33 or len(sig) < 8:
            continue
        r, s = ev.ref.der_decode(sig)
        if r >= 1 << 256 or s >= 1 << 256:
            continue
        low = s <= ev.HALF_N
        plain.append(("ordinary", msg, r.to_bytes(32, "big") + s.to_bytes(32, "big"), pub, ok and low))
    front = (-n) % 64
    assert len(plain) >= front
    backwards = plain[:front] + comp[::-1] + [comp[0]]
    for i in range(n):
        assert backwards[front + n - 1 - i][0] == comp[i][0] and ((front + n - 1 - i) % 64 < 32) != (i % 64 < 32)
    forwards = comp + ([comp[0]] if n % 64 == 0 else [])
    old = pin_path(native, path)
    try:
        for how, batch in (("in_order", forwards), ("reversed", backwards)):
            assert len(batch) % 64 != 0
            got = native.gpu_verify_ecdsa_packed(b"".join(c[1] for c in batch), b"".join(c[2] for c in batch),
                                                 b"".join(c[3] for c in batch))
            _check(f"compact, {path}, {how}", [c[0] for c in batch], got, [c[4] for c in batch])
    finally:
        unpin_path(native, old)
