#!/usr/bin/env python3
"""Generate x25519_edge_vectors.tsv: X25519 inputs and field-operation inputs
at the edges where a limb implementation goes wrong while random inputs and
the RFC vectors pass.  Plain Python big integers; every expected value is
computed twice (the x-only ladder below and make_fixtures.x25519) and asserted.

Section 1, one vector per line:   scalar_hex u_hex expected_hex class

  small_out    X25519 outputs 2, 9 and 16: the only way to make the final
               conditional subtraction of fe_tobytes run.  A product that is
               congruent to r in 1..18 leaves the carry pass as p + r, so
               h >= p and q = 1; an output >= 19 has q = 0.  (An all-zero
               output has q = 1 as well, from h = p exactly: the ladder's
               differences are f + 2p - g, so a zero comes as a multiple of p
               in the limbs.  That case the random-input tests already meet;
               it says nothing about where 19 q is added or how the carry of
               h + 19 runs through limbs that are not all ones.)
               u = 9 and 16 lie on the curve with prime
               order l, u = 2 on the twist with prime order l'.  For a clamped
               scalar k let P = [k^-1 mod order] u (unclamped x-only ladder):
               then X25519(k, P) = u, no discrete logarithm needed.  Half of
               the inputs are given non-canonically (bit 255 set; + p too
               where that fits in 255 bits, which a 255-bit P never does).
  near_out     the same construction for every prime-order u in 19..40: the
               other side of the boundary (q = 0).
  noncanonical u = p .. p+18, 2^255-1, 2^256-1.
  low_order    0, 1, p-1, p, p+1 and the two order-8 u (found below as the
               torsion part of random curve points, confirmed by [8]u = O and
               [4]u != O), with and without bit 255, + p where that fits;
               scalars include all-0x00 and all-0xff.  Expected: all zero.
  limb_edges   u = 2^o - 1, 2^o, 2^o + 1 at the limb offsets o of the device's
               radix 2^25.5 (26 51 77 102 128 153 179 204 230; 51, 102, 153,
               204 are the host's 51-bit offsets), scalars with exactly one
               free bit besides the clamp's bit 254: bit 3, bit 253 and the
               bits either side of each 32-bit word boundary.  Every (offset,
               scalar) pair appears once, the three u of an offset taking
               turns, so every u meets at least five scalars.
  base_point   u = 9 with the same one-bit scalars, all-0x00, all-0xff and two
               random ones: the inputs on which the device's fixed-base path
               (base_scalarmult) must agree with its ladder.

Section 2, field operations of x25519_device.hpp at their limb bounds:
    op f0 .. f9 g0 .. g9 expected_hex      (limbs in hex)
  op: mul (f*g), sq (f^2), mul121665, sub_then_sq ((f - g)^2 through fe_sub),
  add_then_mul ((f + g)(f - g) through fe_add and fe_sub: the ladder's d*a),
  tobytes (f).  expected is the canonical value mod p of the integer the
  limbs stand for, sum f_i 2^off_i, so an overflow in 19*g, 38*f or a column
  sum shows as a wrong value.

The limb bound.  fe_carry leaves even limbs <= 2^26 - 1 and odd limbs
<= 2^25 - 1, except h1, which takes the last carry: h1 <= 2^25 - 1 + D with
D = (2^26 - 1 + 19 c9) >> 26 and c9 = t9 >> 25 the carry out of the top column.
Every operand of the ladder's and ge_madd's fe_add / fe_sub is carried (a
product, fe_mul121665, fe_reduce, fe_frombytes or a table entry), and every
product input is carried, a sum of two carried, or f + 2p - g of two carried.
fe_sub's result is the largest: per limb (carried max) + (limb of 2p), i.e.
  limb 0: 2^26 - 1 + 2^27 - 38;  even: 2^26 - 1 + 2^27 - 2 = 3 2^26 - 3;
  odd:    2^25 - 1 + 2^26 - 2 = 3 2^25 - 3;  limb 1: 3 2^25 - 3 + D
(fe_add gives 2^27 - 2 / 2^26 - 2 + 2 D, which is smaller).  D itself depends
on the largest column sum, which depends on the bound: bound() iterates to
the fixed point, and main() prints it with the headroom of 38 * odd limb and
19 * even limb to 2^32 and of the largest column sum to 2^64.
"""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_fixtures  # noqa: E402  (the independent ladder)

P = 2 ** 255 - 19
A = 486662
L_CURVE = 2 ** 252 + 27742317777372353535851937790883648493
L_TWIST = 2 ** 253 - 55484635554744707071703875581767296995
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "x25519_edge_vectors.tsv")
OFFS = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
M255 = 2 ** 255 - 1


def ladder(k, u):
    """[k]u, x-only, k unclamped (< 2^255): projective (X, Z); Z = 0 is O."""
    x1, x2, z2, x3, z3 = u % P, 1, 0, u % P, 1
    for t in reversed(range(255)):
        if (k >> t) & 1:
            x2, x3, z2, z3 = x3, x2, z3, z2
        a, b, c, d = (x2 + z2) % P, (x2 - z2) % P, (x3 + z3) % P, (x3 - z3) % P
        aa, bb, da, cb = a * a % P, b * b % P, d * a % P, c * b % P
        e = (aa - bb) % P
        x3, z3 = (da + cb) ** 2 % P, x1 * (da - cb) ** 2 % P
        x2, z2 = aa * bb % P, e * (aa + 121665 * e) % P
        if (k >> t) & 1:
            x2, x3, z2, z3 = x3, x2, z3, z2
    return x2, z2


def affine(xz):
    return xz[0] * pow(xz[1], P - 2, P) % P


def on_curve(u):
    v2 = (u * u * u + A * u * u + u) % P
    return v2 == 0 or pow(v2, (P - 1) // 2, P) == 1


def prime_order(u):
    """l or l' if u (not 0) generates a subgroup of that prime order, else None."""
    order = L_CURVE if on_curve(u) else L_TWIST
    return order if u % P != 0 and ladder(order, u)[1] == 0 else None


def clamp(sk):
    k = bytearray(sk)
    k[0] &= 248
    k[31] &= 127
    k[31] |= 64
    return int.from_bytes(k, "little")


def le(x):
    return x.to_bytes(32, "little")


def x25519(sk, ub):
    """Expected output: this file's ladder, asserted against make_fixtures'."""
    r = le(affine(ladder(clamp(sk), int.from_bytes(ub, "little") & M255)))
    assert r == make_fixtures.x25519(sk, ub)
    return r


def preimages(rng, u, count):
    """count (scalar, P) with X25519(scalar, P) = u; every other one non-canonical."""
    order = prime_order(u)
    assert order
    out = []
    for j in range(count):
        sk = rng.randbytes(32)
        if j == 0:
            sk = bytes(32)
        if j == 1:
            sk = b"\xff" * 32
        k = clamp(sk)
        assert k % order
        pt = affine(ladder(pow(k, -1, order), u))
        assert prime_order(pt) == order
        if j % 2:
            if pt + P <= M255:
                pt += P
            pt |= 1 << 255
        assert x25519(sk, le(pt)) == le(u), (u, j)
        out.append((sk, le(pt), le(u)))
    return out


def order8_points(rng):
    """The two u of order 8: the l-multiple of a curve point is a torsion
    point; keep those with [8]Q = O, [4]Q != O."""
    found = set()
    while len(found) < 2:
        u = rng.randrange(2, P)
        if not on_curve(u):
            continue
        q = ladder(L_CURVE, u)
        if q[1] == 0:
            continue
        q = affine(q)
        if ladder(8, q)[1] == 0 and ladder(4, q)[1] != 0:
            found.add(q)
    for q in found:  # every multiple by a clamped scalar (8 | k) is O
        assert on_curve(q) and ladder(8, q)[1] == 0 and ladder(4, q)[1] != 0
    return sorted(found)


def one_bit_scalars():
    bits = [3, 253] + [b for w in range(1, 8) for b in (32 * w - 1, 32 * w)]
    out = []
    for b in bits:
        sk = le((1 << 254) | (1 << b))
        assert clamp(sk) == (1 << 254) | (1 << b)
        out.append(sk)
    return out


def section1():
    rng = random.Random(25519)
    rows = []
    for u in (2, 9, 16):
        rows += [r + ("small_out",) for r in preimages(rng, u, 16)]
    near = [u for u in range(19, 41) if prime_order(u)]
    for u in near:
        rows += [r + ("near_out",) for r in preimages(rng, u, 8)]

    def with_scalars(u, cls, extremes):
        for j in range(4):
            sk = rng.randbytes(32)
            if extremes and j == 0:
                sk = bytes(32)
            if extremes and j == 1:
                sk = b"\xff" * 32
            rows.append((sk, le(u), x25519(sk, le(u)), cls))

    for u in list(range(P, P + 19)) + [2 ** 255 - 1, 2 ** 256 - 1]:
        with_scalars(u, "noncanonical", False)
    o8 = order8_points(rng)
    low = []
    for u in [0, 1, P - 1, P, P + 1] + o8:
        for v in (u, u + P):
            if v <= M255 and v not in low:
                low.append(v)
    for u in low:
        for v in (u, u | (1 << 255)):
            n0 = len(rows)
            with_scalars(v, "low_order", True)
            assert all(r[2] == bytes(32) for r in rows[n0:])
    sc = one_bit_scalars()
    for oi, o in enumerate(OFFS[1:]):
        for si, sk in enumerate(sc):
            u = 2 ** o + (oi + si) % 3 - 1
            rows.append((sk, le(u), x25519(sk, le(u)), "limb_edges"))
    for sk in sc + [bytes(32), b"\xff" * 32, rng.randbytes(32), rng.randbytes(32)]:
        rows.append((sk, le(9), x25519(sk, le(9)), "base_point"))
    return rows, near, o8


# ---- section 2: limb bounds -------------------------------------------------
def carried_max(d):
    return [(2 ** 26 - 1 if i % 2 == 0 else 2 ** 25 - 1) + (d if i == 1 else 0) for i in range(10)]


def two_p():
    return [2 ** 27 - 38] + [2 ** 26 - 2 if i % 2 else 2 ** 27 - 2 for i in range(1, 10)]


def mul_columns(f, g):
    """fe_mul's ten 64-bit column sums, as integers (no wrap)."""
    t = [0] * 10
    for i in range(10):
        for j in range(10):
            x = f[i] * g[j]
            if i % 2 and j % 2:
                x *= 2
            if i + j >= 10:
                x *= 19
            t[(i + j) % 10] += x
    return t


def last_carry(t):
    """fe_carry's final carry into h1 for column sums t."""
    t = list(t)
    for i in range(9):
        t[i + 1] += t[i] >> (25 if i % 2 else 26)
        t[i] &= (1 << (25 if i % 2 else 26)) - 1
    return (2 ** 26 - 1 + 19 * (t[9] >> 25)) >> 26


def bound():
    """(per-limb product-input bound, D, largest column sum), at the fixed point."""
    d = 0
    while True:
        b = [c + q for c, q in zip(carried_max(d), two_p())]
        cols = mul_columns(b, b)
        nd = last_carry(cols)
        if nd == d:
            return b, d, max(cols)
        d = nd


def value(limbs):
    return sum(x << o for x, o in zip(limbs, OFFS))


def canonical_limbs(x):
    return [(x >> o) & ((1 << (25 if i % 2 else 26)) - 1) for i, o in enumerate(OFFS)]


def section2():
    b, d, _ = bound()
    cm = carried_max(d)
    zero = [0] * 10
    shapes = [("bound", b), ("carried", cm), ("alt0", [x if i % 2 == 0 else 0 for i, x in enumerate(b)]),
              ("alt1", [x if i % 2 else 0 for i, x in enumerate(b)])]
    shapes += [("one%d" % i, [b[i] if j == i else 0 for j in range(10)]) for i in range(10)]
    rows = []
    for _, f in shapes:
        rows.append(("sq", f, zero, value(f) ** 2))
        rows.append(("mul121665", f, zero, value(f) * 121665))
        for _, g in shapes[:4]:
            rows.append(("mul", f, g, value(f) * value(g)))
    for i in range(10):  # every single limb against every single limb
        for j in range(10):
            rows.append(("mul", shapes[4 + i][1], shapes[4 + j][1], b[i] * b[j] << (OFFS[i] + OFFS[j])))
    # fe_sub / fe_add take carried operands; f at the carried maximum, g = 0
    # reaches the bound
    one_hot = [[cm[i] if j == i else 0 for j in range(10)] for i in range(10)]
    for f, g in [(cm, zero), (zero, cm), (cm, cm), (canonical_limbs(P - 1), zero)] + \
                [(cm, h) for h in one_hot] + [(h, zero) for h in one_hot]:
        rows.append(("sub_then_sq", f, g, (value(f) - value(g)) ** 2))
        rows.append(("add_then_mul", f, g, (value(f) + value(g)) * (value(f) - value(g))))
    high_h1 = canonical_limbs(P - 1)
    high_h1[1] += d  # carried representation with h1 above 2^25
    for f in [canonical_limbs(x) for x in (P - 1, P, P + 1, P + 18, 2 ** 255 - 1, 0, 1, 18, 19)] + \
             [two_p(), high_h1, cm, b, [x if i != 1 else 2 ** 25 + d - 1 for i, x in enumerate(zero)]]:
        rows.append(("tobytes", f, zero, value(f)))
    assert value(two_p()) == 2 * P and value(canonical_limbs(P + 18)) == P + 18
    for r in rows:
        assert all(0 <= x < 2 ** 32 for x in r[1] + r[2])
    return [(op, f, g, le(v % P)) for op, f, g, v in rows]


def render():
    rows, near, o8 = section1()
    lines = ["# generated by make_x25519_edges.py; do not edit",
             "# section 1: scalar u expected class"]
    lines += ["%s %s %s %s" % (s.hex(), u.hex(), e.hex(), c) for s, u, e, c in rows]
    lines.append("# section 2: op f0..f9 g0..g9 expected")
    for op, f, g, e in section2():
        lines.append(" ".join([op] + ["%x" % x for x in f + g] + [e.hex()]))
    return "\n".join(lines) + "\n", near, o8


def main():
    text, near, o8 = render()
    with open(OUT, "w") as f:
        f.write(text)
    b, d, col = bound()
    import math
    print("prime-order u in 19..40:", near)
    print("order-8 u:", [le(u).hex() for u in o8])
    print("product-input bound per limb:", ["%x" % x for x in b])
    print("  even limbs <= 2^%.4f, odd limbs <= 2^%.4f, last carry into h1 D = %d"
          % (math.log2(max(b[0::2])), math.log2(max(b[1::2])), d))
    print("  38 * odd limb <= 2^%.4f (2^32 / 38 = %d, largest odd limb %d: headroom x%.4f)"
          % (math.log2(38 * max(b[1::2])), 2 ** 32 // 38, max(b[1::2]), 2 ** 32 / 38 / max(b[1::2])))
    print("  19 * even limb <= 2^%.4f (headroom x%.4f)"
          % (math.log2(19 * max(b[0::2])), 2 ** 32 / 19 / max(b[0::2])))
    print("  largest column sum 2^%.4f (headroom to 2^64 x%.4f)" % (math.log2(col), 2 ** 64 / col))
    print("wrote %s: %d lines" % (OUT, text.count("\n")))


if __name__ == "__main__":
    main()
