"""Constructed ECDSA edge-case vectors for the verifiers (csrc/secp256k1/secp256k1.cpp on the CPU,
csrc/kernels/secp256k1.hip on the MI355X), judged by the pure-Python oracle.

A plain helper module (imported by tests/test_ecdsa_vectors.py, like test_ecdsa_der_gpu.py imports
test_ecdsa_batch). `build()` makes the vectors once per process. Each vector is
(label, pubkey bytes, DER signature, msg32, expected verdict); the expected verdict is written down
by construction where the vector is made, and `_Builder.add` asserts it against
ref.verify(..., require_low_s=False) on what ref.der_decode reads back from the signature, so a
construction that does not do what its label says fails here, on the CPU, before any kernel runs.
Nothing in here asks the code under test for a verdict, a signature or a key.

Three constructions reach scalars and points that random signing reaches with probability 2^-128
(docs/ECDSA_VECTORS.md):
  * ref.forge(u1, u2, Q): a valid signature under any curve point Q for which the verifier computes
    exactly the chosen u1 and u2 (an ECDSA verifier can be handed any pair);
  * ref.recover_with(R, r, s, msg): the key under which the verifier's u1*G + u2*Q is a chosen R,
    which gives signatures with x(R) in [n, p) and the invalid ones just past that boundary;
  * ref.sign_with(k, d, s): the message that makes a chosen s valid (the inverse's input).
Everything is drawn from one fixed seed.
"""
import collections
import random
import time

from bitcoincashplus_amd.utils import secp256k1_ref as ref

N, P = ref.N, ref.P
SEED = 0xEC05A
HALF_N = N // 2

Vector = collections.namedtuple("Vector", "label pub sig msg expect")

# The family sizes the issue asks for at the least (tests/test_ecdsa_vectors.py checks them).
MIN_COUNTS = {"A": 30, "B": 75, "C": 9, "D": 140, "E": 75}

# lattice basis of {(a, b): a + b*lambda = 0 (mod n)} behind the kernel's GLV_A1, GLV_B1N, GLV_A2,
# GLV_B2 (b1 = -GLV_B1N)
GLV_A1 = 0x3086D221A7D46BCDE86C90E49284EB15
GLV_B1 = -0xE4437ED6010E88286F547FA90ABFE4C3
GLV_A2 = 0x114CA50F7A8E2F3F657C1108D9D44CFD8
GLV_B2 = GLV_A1


def _round_div(a, b):
    return (2 * a + b) // (2 * b)


def glv_split(k):
    """(k1, k2) with k = k1 + k2*lambda (mod n): k minus the lattice vector nearest to (k, 0) by
    rounding, the split the kernels aim for (theirs rounds through 2^384-scaled constants and may
    differ by one lattice vector; the oracle, not this split, decides every verdict)."""
    c1 = _round_div(GLV_B2 * k, N)
    c2 = _round_div(-GLV_B1 * k, N)
    k1 = k - c1 * GLV_A1 - c2 * GLV_A2
    k2 = -c1 * GLV_B1 - c2 * GLV_B2
    assert (k1 + k2 * ref.LAMBDA - k) % N == 0
    return k1, k2


def _neg(pt):
    return (pt[0], P - pt[1])


def _pub(pt, form="compressed"):
    if form == "compressed":
        return ref.serialize_pubkey(pt, True)
    raw = ref.serialize_pubkey(pt, False)
    if form == "uncompressed":
        return raw
    parity = pt[1] & 1
    if form == "hybrid":
        return bytes([6 + parity]) + raw[1:]
    if form == "hybrid_wrong":
        return bytes([7 - parity]) + raw[1:]
    raise ValueError(form)


class _Builder:
    def __init__(self):
        self.rng = random.Random(SEED)
        self.vectors = []
        self.compact_expect = {}  # label -> verdict of the compact (low-S only) entry point
        self.retries = 0          # forgeries thrown away because s came out high
        self.oracle_calls = 0

    def add(self, label, pub, r, s, msg, expect):
        assert len(msg) == 32 and label not in self.compact_expect, label
        sig = ref.der_encode(r, s)
        assert len(sig) <= 72, label
        rr, ss = ref.der_decode(sig)
        assert (rr, ss) == (r, s), label
        # with a low s the strict call is the lax one; with a high s the strict call costs nothing
        strict = ref.verify(pub, rr, ss, msg, require_low_s=True)
        got = strict if ss <= HALF_N else ref.verify(pub, rr, ss, msg, require_low_s=False)
        self.oracle_calls += 1
        assert got == expect, f"{label}: constructed as {expect}, the oracle says {got}"
        self.vectors.append(Vector(label, pub, sig, msg, expect))
        self.compact_expect[label] = strict

    def scalar(self):
        return self.rng.randrange(1, N)

    def low_s(self):
        return self.rng.randrange(1, HALF_N + 1)

    def msg(self):
        return self.rng.randbytes(32)

    def forge_low(self, Q, u1=None, u2=None):
        """ref.forge with the scalar that is None drawn from the seed, again until s <= n/2, so
        that the verifier (which normalises a high s) works with the named scalars, not their
        negatives. Returns (r, s, msg)."""
        while True:
            a = self.scalar() if u1 is None else u1
            b = self.scalar() if u2 is None else u2
            r, s, msg = ref.forge(a, b, Q)
            if s <= HALF_N:
                return r, s, msg
            self.retries += 1
            assert u1 is None or u2 is None, "nothing left to draw again"


def _on_curve_from(start, step, count):
    xs, x = [], start
    while len(xs) < count:
        if ref.lift_x(x, 0) is not None:
            xs.append(x)
        x += step
    return xs


# ---------------------------------------------------------------- A: x(R) >= n
def _family_a(b):
    above_n = _on_curve_from(N + 1, 1, 5)
    below_p = _on_curve_from(P - 1, -1, 5)
    assert above_n == [N + 2, N + 4, N + 6, N + 7, N + 9]
    assert below_p == [P - 3, P - 4, P - 10, P - 12, P - 13]
    for x in above_n + below_p:
        for odd in (0, 1):
            # r = x - n is small or just under p - n; the verifier has to compare with r + n
            R = ref.lift_x(x, odd)
            r, s, msg = x - N, b.low_s(), b.msg()
            name = f"n+{x - N}" if x - N < 100 else f"p-{P - x}"
            b.add(f"A.xR_ge_n.{name}.{'odd' if odd else 'even'}", _pub(ref.recover_with(R, r, s, msg)), r, s, msg, True)
    for x in (1, 2, 3):
        # x(R) = r small, r + n < p as well: the first compare matches
        R = ref.lift_x(x, x & 1)
        s, msg = b.low_s(), b.msg()
        b.add(f"A.xR_small.{x}", _pub(ref.recover_with(R, x, s, msg)), x, s, msg, True)
    for x0 in (1, 2, 3, 4):
        for odd in (0, 1):
            # r + n = p + x0 is x0 modulo p but no x coordinate: r + n < p must be checked
            R = ref.lift_x(x0, odd)
            r, s, msg = P - N + x0, b.low_s(), b.msg()
            b.add(f"A.r_plus_n_wraps.{x0}.{'odd' if odd else 'even'}", _pub(ref.recover_with(R, r, s, msg)), r, s, msg, False)
    for name, r in (("p-n-1", P - N - 1), ("p-n", P - N)):
        R = ref.point_mul(b.scalar())
        s, msg = b.low_s(), b.msg()
        b.add(f"A.r_boundary.{name}", _pub(ref.recover_with(R, r, s, msg)), r, s, msg, False)


# ---------------------------------------------------------------- B: chosen u1, u2
def _u1_cases():
    cases = collections.OrderedDict()
    cases["0"] = 0  # the all-zero message: every comb window is skipped
    for i in (0, 15, 31):
        for v in (1, 255):
            cases[f"byte{i}x{v}"] = v << (8 * i)
    for i in (0, 11, 12, 23):
        for w in ((1, 7) if i == 23 else (1, 2047)):
            cases[f"win{i}x{w}"] = w << (11 * i)
    cases["n-1"] = N - 1
    cases["n-2"] = N - 2
    cases["(n-1)/2"] = (N - 1) // 2
    cases["2^255"] = 1 << 255
    assert all(0 <= v < N for v in cases.values())
    return cases


def _u2_cases(rng):
    lam = ref.LAMBDA
    cases = collections.OrderedDict()
    for v in (1, 2, 3, 15, 16, 17):
        assert glv_split(v) == (v, 0)
        cases[f"{v}"] = v  # second GLV half 0
    for j in (1, 2, 3):
        assert glv_split(j * lam % N) == (0, j)
        cases[f"{j}*lambda"] = j * lam % N  # first GLV half 0
    cases["n-1"] = N - 1
    cases["n-2"] = N - 2
    cases["n-lambda"] = N - lam
    mags = [0, 1, 2, 15, 16, 1 << 64, (1 << 127) - 1, 1 << 127]
    signed = [0] + [sg * m for m in mags[1:] for sg in (1, -1)]
    top = [(1 << 127) - 1, 1 << 127, -((1 << 127) - 1), -(1 << 127)]
    # the corners (both halves at their largest, every sign), then a seeded draw of the rest
    pairs = [(k1, k2) for k1 in top for k2 in top] + [(k, 0) for k in top] + [(0, k) for k in top]
    rest = [(k1, k2) for k1 in signed for k2 in signed if (k1, k2) != (0, 0) and (k1, k2) not in pairs]
    pairs += rng.sample(rest, 40 - len(pairs))

    def fmt(k):
        return {(1 << 127) - 1: "2^127-1", 1 << 127: "2^127", 1 << 64: "2^64"}.get(abs(k), str(abs(k)))

    for k1, k2 in pairs:
        label = f"{'-' if k1 < 0 else '+'}{fmt(k1)}{'-' if k2 < 0 else '+'}{fmt(k2)}*lambda"
        cases[label] = (k1 + k2 * lam) % N
    a1, a2 = GLV_A1, GLV_A2
    for label, v in (("a1", a1), ("-a1", -a1), ("2*a1", 2 * a1), ("-2*a1", -2 * a1), ("a1+a2", a1 + a2),
                     ("a2", a2), ("-b1", -GLV_B1)):
        cases[label] = v % N
    ones = lambda nib: int(nib * 32, 16)  # noqa: E731
    octal = lambda d: int(d * 42, 8)  # noqa: E731
    for label, h in (("nibF", ones("f")), ("nib1", ones("1")), ("nib8", ones("8")), ("nib7", ones("7")),
                     ("oct7", octal("7")), ("oct4", octal("4"))):
        cases[f"{label}+{label}*lambda"] = (h + h * lam) % N
    assert all(0 < v < N for v in cases.values()) and len(set(cases.values())) == len(cases)
    return cases


def _family_b(b):
    pool = [ref.point_mul(b.scalar()) for _ in range(4)]
    for i, (label, u1) in enumerate(_u1_cases().items()):
        Q = pool[i % 4]
        r, s, msg = b.forge_low(Q, u1=u1)
        if u1 == 0:
            assert msg == bytes(32)
        b.add(f"B.u1.{label}", _pub(Q), r, s, msg, True)
    for i, (label, u2) in enumerate(_u2_cases(b.rng).items()):
        Q = pool[i % 4]
        r, s, msg = b.forge_low(Q, u2=u2)
        b.add(f"B.u2.{label}", _pub(Q), r, s, msg, True)


# ---------------------------------------------------------------- C: chosen s
def _family_c(b):
    lows = collections.OrderedDict([("1", 1), ("2", 2), ("3", 3), ("2^128", 1 << 128),
                                    ("n-2^255", N - (1 << 255)), ("(n-1)/2", (N - 1) // 2)])
    assert all(0 < s <= HALF_N for s in lows.values()) and (1 << 255) > HALF_N
    for name, s in lows.items():
        for rep in range(2):
            k, d = b.scalar(), b.scalar()
            r, _, msg = ref.sign_with(k, d, s)
            pub = _pub(ref.point_mul(d))
            b.add(f"C.s.{name}.{rep}", pub, r, s, msg, True)
            if rep == 0 and name in ("1", "2^128", "n-2^255", "(n-1)/2"):
                # the high twin: valid through CPubKey::Verify (it normalises s), not for a
                # verifier of compact low-S signatures
                b.add(f"C.twin.n-({name})", pub, r, N - s, msg, True)
                assert b.compact_expect[f"C.twin.n-({name})"] is False


# ---------------------------------------------------------------- D: Q related to G
DOUBLING_CANDIDATES = (1, 3, 5, 255, 2047, 1 << 11, 3 << 88)
EQUAL_HALVES_CANDIDATES = (1, 3, 5, 255, 2047, 1 << 11, 3 << 88, 1 << 121)  # within comb windows 0-11


def _family_d(b):
    lam = ref.LAMBDA
    lamG = ref.point_mul(lam)
    assert lamG == (ref.BETA * ref.G[0] % P, ref.G[1])
    related = collections.OrderedDict([("G", (1, ref.G)), ("-G", (N - 1, _neg(ref.G))), ("2G", (2, ref.point_mul(2))),
                                       ("lambdaG", (lam, lamG)), ("-lambdaG", (N - lam, _neg(lamG)))])
    # u1 = u2 = a, one comb window, Q = G: u2*Q = a*G, and the comb then adds a*G to it (P + P)
    kept = 0
    for a in DOUBLING_CANDIDATES:
        r, s, msg = ref.forge(a, a, ref.G)
        if s > HALF_N:  # the verifier would work with (-a, -a): not one window
            b.retries += 1
            continue
        kept += 1
        b.add(f"D.double.G.{a:#x}", _pub(ref.G), r, s, msg, True)
    b.kept_doubling = kept
    assert kept >= 3, kept
    # a comb of two windows whose first addition meets u2*Q: a*G + a*G (Q = G), a*G - a*G (Q = -G)
    for a in (1, 5, 2047):
        for qn in ("G", "-G"):
            r, s, msg = ref.forge(a + (1 << 200), a if qn == "G" else N - a, related[qn][1])
            b.add(f"D.first_window.{qn}.{a}", _pub(related[qn][1]), r, s, msg, True)
    # Q = lambda^2*G, so lambda*Q = G. u2 = a*lambda splits into (0, a): the first half of u2*Q is
    # the point at infinity and the second is a*G. With u1 = a in the low comb windows, the two
    # partial points that the fused and the half-lane kernel add at the very end are both a*G
    # (Jacobian + Jacobian doubling); under -Q they cancel. Nothing is drawn from the seed here.
    lam2G = ref.point_mul(lam * lam % N)
    kept = 0
    for a in EQUAL_HALVES_CANDIDATES:
        assert glv_split(a * lam % N) == (0, a)
        r, s, msg = ref.forge(a, a * lam % N, lam2G)
        if s > HALF_N:
            b.retries += 1
            continue
        kept += 1
        b.add(f"D.equal_halves.{a:#x}", _pub(lam2G), r, s, msg, True)
        r0 = 1000 + a
        while r0 * pow(a * lam, -1, N) % N > HALF_N:
            r0 += 1
        r, s, msg = ref.forge(a, a * lam % N, _neg(lam2G), r=r0)
        b.add(f"D.opposite_halves.{a:#x}", _pub(_neg(lam2G)), r, s, msg, False)
    b.kept_equal_halves = kept
    assert kept >= 3, kept
    grid = (1, 2, 3, N - 1, N - 2)
    gname = {1: "1", 2: "2", 3: "3", N - 1: "n-1", N - 2: "n-2"}
    for qn, (d, Q) in related.items():
        for u1 in grid:
            for u2 in grid:
                label = f"D.grid.{qn}.{gname[u1]}.{gname[u2]}"
                if (u1 + d * u2) % N == 0:
                    # R is the point at infinity: no r verifies. s = r/u2 follows from r; the seeded
                    # r is drawn until that s is low (with r = 1 it is what it is: -R is infinite too)
                    while True:
                        rr = b.scalar()
                        if rr * pow(u2, -1, N) % N <= HALF_N:
                            break
                    for rname, r0 in (("r1", 1), ("rseed", rr)):
                        r, s, msg = ref.forge(u1, u2, Q, r=r0)
                        b.add(f"{label}.inf.{rname}", _pub(Q), r, s, msg, False)
                else:
                    r, s, msg = ref.forge(u1, u2, Q)
                    b.add(label, _pub(Q), r, s, msg, True)
    # seeded (r, s) with z such that u1 + d*u2 = (z + r*d)/s = 0: R is the point at infinity
    for qn in ("2G", "lambdaG"):
        d, Q = related[qn]
        for i in range(6):
            r, s = b.scalar(), b.low_s()
            b.add(f"D.cancel.{qn}.{i}", _pub(Q), r, s, ((-r * d) % N).to_bytes(32, "big"), False)


# ---------------------------------------------------------------- E: keys
def _family_e(b):
    small = [1, 2, 3, 4]
    large = _on_curve_from(P - 1, -1, 4)
    assert all(ref.lift_x(x, 0) is not None for x in small) and large == [P - 3, P - 4, P - 10, P - 12]
    good = None
    for x in small + large:
        for odd in (0, 1):
            Q = ref.lift_x(x, odd)
            r, s, msg = b.forge_low(Q)
            name = f"{x}" if x < 100 else f"p-{P - x}"
            tag = f"{name}.{'odd' if odd else 'even'}"
            b.add(f"E.compressed.{tag}", _pub(Q), r, s, msg, True)
            b.add(f"E.uncompressed.{tag}", _pub(Q, "uncompressed"), r, s, msg, True)
            b.add(f"E.hybrid.{tag}", _pub(Q, "hybrid"), r, s, msg, True)
            b.add(f"E.hybrid_wrong_parity.{tag}", _pub(Q, "hybrid_wrong"), r, s, msg, False)
            if x in small:
                # x + p names the same residue; a key is only valid with x < p
                alias = bytes([2 + odd]) + (P + x).to_bytes(32, "big")
                b.add(f"E.alias_x_plus_p.{tag}", alias, r, s, msg, False)
            good = (Q, r, s, msg)
    Q, r, s, msg = good
    xq = Q[0].to_bytes(32, "big")
    b.add("E.x_is_p", b"\x02" + P.to_bytes(32, "big"), r, s, msg, False)
    b.add("E.x_is_2^256-1", b"\x03" + b"\xff" * 32, r, s, msg, False)
    off = [x for x in range(5, 12) if ref.lift_x(x, 0) is None][:4]
    assert len(off) == 4
    for x in off:
        b.add(f"E.off_curve.{x}", bytes([2 + (x & 1)]) + x.to_bytes(32, "big"), r, s, msg, False)
    for prefix in (0, 4, 5):
        b.add(f"E.prefix_{prefix:02x}_33_bytes", bytes([prefix]) + xq, r, s, msg, False)


_FAMILIES = (("A", _family_a), ("B", _family_b), ("C", _family_c), ("D", _family_d), ("E", _family_e))
_built = None


def build():
    """The vectors, built once per process: an object with .vectors (list of Vector), .family(name),
    .compact (the entries the compact entry point can take), .retries (high-s forgeries drawn
    again or, for family D's doubling and equal-halves candidates, left out), .kept_doubling,
    .kept_equal_halves and .seconds."""
    global _built
    if _built is None:
        t0 = time.perf_counter()
        b = _Builder()
        for _, make in _FAMILIES:
            make(b)
        b.seconds = time.perf_counter() - t0
        labels = [v.label for v in b.vectors]
        assert len(set(labels)) == len(labels)
        _built = _Vectors(b)
    return _built


class _Vectors:
    def __init__(self, b):
        self.vectors = tuple(b.vectors)
        self.retries = b.retries
        self.kept_doubling = b.kept_doubling
        self.kept_equal_halves = b.kept_equal_halves
        self.oracle_calls = b.oracle_calls
        self.seconds = b.seconds
        # (label, msg32, r || s, pub33, verdict) for the entry point that takes compact low-S
        # signatures and compressed keys: every vector with a 33-byte key and a low s, and family
        # C's high twins (invalid there). The verdicts are the oracle's with require_low_s=True.
        compact = []
        for v in self.vectors:
            r, s = ref.der_decode(v.sig)
            if len(v.pub) == 33 and (s <= HALF_N or v.label.startswith("C.twin.")):
                compact.append((v.label, v.msg, r.to_bytes(32, "big") + s.to_bytes(32, "big"), v.pub,
                                b.compact_expect[v.label]))
        self.compact = tuple(compact)

    def family(self, name):
        return [v for v in self.vectors if v.label.startswith(name + ".")]
