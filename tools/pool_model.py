"""Limb-level model of the obfuscator-pool kernels (ibond-flex_amd/csrc/kernels_pool.hpp): k_pool_split, k_pool_join and
the arithmetic of k_pool_enc, in 28-bit limbs, 37 per lane, with the kernels' lazy 64-bit accumulators and their bounds
asserted. For checking the algebra on the host before the kernels change; tests/test_pool_model.py compares it with
Python integers. Run directly for a self-check: python tools/pool_model.py

With rho = a + n b, a, b < n:   (1 + n M) rho = a + n ((b + M a) mod n)   (mod n^2).

A ring row holds (a', b), a' = a 2^84 mod n. The chosen reduction of |M| a mod n is Montgomery's: three digit steps
over the three 28-bit limbs of |M| against a', a' |M| 2^-84 mod n, below 2 n before one conditional subtraction; a comes
back from three reduction steps over a' alone. Every value mod n is an S-limb operand of the whole lane group
(S = 37 TPI; n's limbs above its own are zero).
"""
import random

LB = 28
MASK = (1 << LB) - 1
L = 37
U64 = 1 << 64


def tpi_for(nbits):
    """Lanes per group of the encrypt engine (pai_ctx_create: n^2 and two spare bits must fit 28 * 37 * TPI bits)."""
    for t in (2, 4, 8):
        if LB * L * t >= 2 * nbits + 2:
            return t
    raise ValueError("key size not supported")


def limbs(x, S):
    assert 0 <= x < 1 << (LB * S)
    return [(x >> (LB * i)) & MASK for i in range(S)]


def val(l):
    return sum(v << (LB * i) for i, v in enumerate(l))


def normalize(P, drop_carry=False):
    """bn_group.hpp normalize: lazy accumulators -> canonical limbs. The carry out of the top limb does not exist (the
    total is below 2^(28 S)) unless the caller adds n to a wrapped difference, where it is dropped."""
    out, c = [], 0
    for v in P:
        assert 0 <= v < U64
        v += c
        assert v < U64
        out.append(v & MASK)
        c = v >> LB
    assert drop_carry or c == 0
    return out


def sub_limbs(a, b):
    """bn_group.hpp sub_limbs: (a - b mod 2^(28 S), borrow)."""
    S = len(a)
    d = val(a) - val(b)
    return limbs(d % (1 << (LB * S)), S), d < 0


def cond_sub(r, m):
    d, neg = sub_limbs(r, m)
    return r if neg else d


def shift_down(P):
    """The one-limb shift of the CIOS loops: every accumulator moves down one place inside its lane; a lane's lowest
    accumulator hands its low 28 bits to the previous lane's top place and keeps the rest for its next one (the
    group's lowest is 0 mod 2^28 after the reduction step; the top place receives 0)."""
    S = len(P)
    low = [P[t] for t in range(0, S, L)]
    P[:] = P[1:] + [0]
    for t, v in enumerate(low):
        P[t * L] += v >> LB
        if t:
            P[t * L - 1] = v & MASK


def digit_step(P, a, d, m, nprime):
    """pool_digit: P <- (P + a d + q n) / 2^28, q = -P_0 n^-1 mod 2^28, on lazy accumulators: the low limb's upper bits
    stay with the next accumulator, as in the kernel (the lanes' one-limb shift moves 28 bits)."""
    if a is not None:
        P[:] = [p + x * d for p, x in zip(P, a)]
    q = ((P[0] & 0xFFFFFFFF) * nprime) & MASK
    P[:] = [p + q * x for p, x in zip(P, m)]
    assert max(P) < U64 and P[0] & MASK == 0
    shift_down(P)


def mont_reduce(P, m, mprime, collect=None):
    """bn_group.hpp cios<AB = false>: S reduction steps; collect: the quotient digits (exact division)."""
    S = len(P)
    for j in range(S):
        q = ((P[0] & 0xFFFFFFFF) * mprime) & MASK
        if collect is not None:
            collect[j] = q
        P[:] = [p + q * x for p, x in zip(P, m)]
        assert max(P) < U64 and P[0] & MASK == 0
        shift_down(P)


def montmul(a, b, m, mprime):
    """bn_group.hpp montmul: a b R^-1 mod m, below 2 m, canonical limbs."""
    S = len(a)
    P = [0] * S
    for j in range(S):
        bj = b[j]
        P[:] = [p + x * bj for p, x in zip(P, a)]
        q = ((P[0] & 0xFFFFFFFF) * mprime) & MASK
        P[:] = [p + q * x for p, x in zip(P, m)]
        assert max(P) < U64
        shift_down(P)
    return normalize(P)


class Key:
    """The constants pai_pool_reserve uploads (flexpai.hip pool_consts)."""

    def __init__(self, n):
        self.n = n
        self.nbits = n.bit_length()
        self.tpi = tpi_for(self.nbits)
        self.S = L * self.tpi
        self.R = 1 << (LB * self.S)
        self.nl = limbs(n, self.S)
        assert self.nbits <= LB * self.S // 2 - 1     # n, and every value below n, fits half of the group's limbs
        self.nprime = (-pow(n, -1, 1 << LB)) % (1 << LB)
        self.nneg = limbs(self.R - n, self.S)
        self.dprime = (-pow(self.R - n, -1, 1 << LB)) % (1 << LB)
        self.R2n = limbs(self.R * self.R % n, self.S)
        self.R2n84 = limbs((self.R * self.R << (3 * LB)) % n, self.S)
        self.pt_words = -(-self.nbits // 32)
        self.ct_words = -(-2 * self.nbits // 32)


def split(k, rho):
    """k_pool_split: rho < n^2 -> the ring row (a', b) as integers below 2^(32 pt_words)."""
    assert 0 <= rho < k.n * k.n
    x = limbs(rho, k.S)
    P = list(x)
    mont_reduce(P, k.nl, k.nprime)
    u = normalize(P)                                  # rho R^-1 mod n, below 2 n
    assert val(u) < 2 * k.n
    ap = cond_sub(montmul(u, k.R2n84, k.nl, k.nprime), k.nl)
    a = cond_sub(montmul(u, k.R2n, k.nl, k.nprime), k.nl)
    d, neg = sub_limbs(x, a)
    assert not neg
    b = [0] * k.S
    P = list(d)
    mont_reduce(P, k.nneg, k.dprime, collect=b)
    ap, b = val(ap), val(b)
    assert ap < k.n and b < k.n
    return ap, b


def apply(k, row, M):
    """pool_apply: (1 + n M) rho mod n^2 from rho's row, M the encoder's int64."""
    ap_i, b_i = row
    assert -(1 << 63) <= M < 1 << 63
    S = k.S
    ap, b = limbs(ap_i, S), limbs(b_i, S)
    neg = M < 0
    mag = -M if neg else M
    Md = [mag & MASK, (mag >> LB) & MASK, mag >> (2 * LB)]
    P = [0] * S
    for d in Md:
        digit_step(P, ap, d, k.nl, k.nprime)
    w = normalize(P)
    assert val(w) < 2 * k.n
    w = cond_sub(w, k.nl)
    s = cond_sub(normalize([b[i] + w[i] for i in range(S)]), k.nl)
    d, borrow = sub_limbs(b, w)
    d = normalize([d[i] + (k.nl[i] if borrow else 0) for i in range(S)], drop_carry=True)
    tp = d if neg else s
    assert val(tp) < k.n
    P = list(ap)
    for _ in range(3):
        digit_step(P, None, 0, k.nl, k.nprime)
    a = normalize(P)
    assert val(a) < 2 * k.n
    a = cond_sub(a, k.nl)
    # c = a + n t' by rows (pool_prod_step): after digit j the limb that leaves at the bottom is limb j of c and replaces
    # the digit in the slot; the accumulators end as the high half
    P, slot = list(a), list(tp)
    assert all(v == 0 for v in tp[S // 2:])
    for j in range(S // 2):
        bj = slot[j]
        P = [p + x * bj for p, x in zip(P, k.nl)]
        assert max(P) < 1 << 62
        slot[j] = P[0] & MASK
        P[0] -= slot[j]                               # the group's lowest lane hands nothing down
        shift_down(P)
    hi = normalize(P)
    assert all(v == 0 for v in hi[S // 2:])
    c = val(slot[:S // 2] + hi[:S // 2])
    assert c < k.n * k.n
    return c


def join(k, row):
    """k_pool_join: the plain rho of a row."""
    return apply(k, row, 0)


def mac_counts(S):
    """Multiply-accumulates per element: the pooled product, and make_c0 + k_obf_mul's two Montgomery products."""
    return {"pool_enc": (S // 2) ** 2 + 9 * (S // 2), "c0_obf_mul": 4 * S * S + 3 * S}


if __name__ == "__main__":
    rng = random.Random(1)
    for nbits in (512, 1035, 2048):
        p = rng.getrandbits(nbits // 2) | (1 << (nbits // 2 - 1)) | 1
        q = rng.getrandbits(nbits - nbits // 2) | (1 << (nbits - nbits // 2 - 1)) | 1
        k = Key(p * q)
        n2 = k.n * k.n
        for _ in range(4):
            rho = rng.randrange(n2)
            M = rng.randrange(-(1 << 63) + 1, 1 << 63)
            row = split(k, rho)
            assert join(k, row) == rho
            assert apply(k, row, M) == (1 + k.n * M) * rho % n2
        print(nbits, "bits: TPI", k.tpi, "ok;", mac_counts(k.S))
