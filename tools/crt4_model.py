"""Limb-level model of the split-pair CRT encryption of a 2049..4096-bit key holder (kernels_crt4.hpp), CPU only.
Not test infrastructure for the product's kernels; run directly (python tools/crt4_model.py) or through
tests/test_crt4_model.py.

Per half h (p = p_h, q = the other prime, S = 74 limbs of 28 bits, R = 2^(28 S)):

  k_crt4_pre  x~ = r R mod p: K passes over r's chunks of S digits against R^(K+1) mod p, the running value normalised
              between passes (T < a + p < 2p)
  k_crt4_a    the lane machine's op list over q mod (p - 1) on one lane: squares on bn_lane.hpp's triangle, products
              one CIOS pass over the multiplier's digits; no closing product: y R mod p (< 2p)
  k_crt4_b    the pair (y R mod p, 0) through d4r_run's op list over p (kernels_dec4.hpp: the even lane holds A, the odd
              lane B; a square is one split pass, a product two), the closing product with the plain pair of the CRT
              coefficient, the canonical pair, u = A + p B over 2 S limbs
  k_crt_fin   (u_p q^2 + u_q p^2) mod n^2 = r^n mod n^2                                           (kernels_crt.hpp)

Two levels. The limb functions do the kernels' arithmetic digit by digit, with every 64-bit accumulator's largest value
recorded; the value functions compute the same integers (the same representatives, not only the same residues) from
REDC's closed form, and run the ~2400-op chains in milliseconds. selfcheck() ties the two together on random and on
extreme operands; run() executes a whole element on the value level, with the passes around the hand-offs (the chunked
reduction, the first ops of each chain, the coefficient product, the canonical pair, the wide product) also on the limb
level, and checks

  - the values against pow();
  - every accumulator below 2^64;
  - the operand bounds the split-pair passes assume: < 2p into a square, a product's result < 4p (its A part < 2p),
    R >= 2^24 p.
"""
import random

LB = 28
MASK = (1 << LB) - 1
S = 74
R = 1 << (LB * S)
KMAX_CHUNKS = 5


def limbs(x, n=S):
    assert 0 <= x < 1 << (LB * n), "value does not fit its limbs"
    return [(x >> (LB * i)) & MASK for i in range(n)]


def val(l):
    return sum(v << (LB * i) for i, v in enumerate(l))


class Track:
    """largest value any 64-bit accumulator held"""
    def __init__(self):
        self.mx = 0

    def see(self, P):
        self.mx = max(self.mx, max(P))
        assert self.mx < 1 << 64, "a 64-bit accumulator overflowed"


def normalize(P):
    c, r = 0, []
    for v in P:
        v += c
        r.append(v & MASK)
        c = v >> LB
    assert c == 0, "the normalised value does not fit S limbs"
    return r


# ---------------------------------------------------------------- limb level
def lane_pass(P, a, dig, pl, pinv, tr, q1s=None, drop=None):
    """d4_pass (kernels_dec4.hpp) on one lane: P += a dig_J + q p per digit, the lowest position retired. q1s: out, the
    reduction digits. drop: the even neighbour's digits (the odd lane of a pair pass, subq): q is taken from P_J - q1 and
    the retiring shift drops q1."""
    for J in range(S):
        y = dig[J]
        for i in range(S):
            P[(i + J) % S] += a[i] * y
        low = P[J] & 0xFFFFFFFF
        if drop is not None:
            low = (low - drop[J]) & 0xFFFFFFFF
        q = (low * pinv) & MASK
        if q1s is not None:
            q1s.append(q)
        for i in range(S):
            P[(i + J) % S] += q * pl[i]
        tr.see(P)
        assert P[J] & MASK == (drop[J] if drop is not None else 0)
        P[(J + 1) % S] += P[J] >> LB
        P[J] = 0
    return P


def lane_sqr(a, pl, pinv, tr):
    """lane::mont_sqr (bn_lane.hpp): the triangle a_i a_j, i >= j, doubled off the diagonal"""
    P = [0] * S
    for J in range(S):
        P[(2 * J) % S] += a[J] * a[J]
        for i in range(J + 1, S):
            P[(i + J) % S] += a[i] * (2 * a[J])
        q = ((P[J] & 0xFFFFFFFF) * pinv) & MASK
        for i in range(S):
            P[(i + J) % S] += q * pl[i]
        tr.see(P)
        assert P[J] & MASK == 0
        P[(J + 1) % S] += P[J] >> LB
        P[J] = 0
    return normalize(P)


def pair_sqr(A, B, x1, pl, pinv, tr):
    """d4r_sqr_step: the even lane P += A A_J, the odd lane P += B 2 A_J from (1 - R) mod p, + LMASK - q1 per digit"""
    Pe, Po = [0] * S, list(x1)
    for J in range(S):
        for i in range(S):
            Pe[(i + J) % S] += A[i] * A[J]
            Po[(i + J) % S] += B[i] * (2 * A[J])
        q1 = ((Pe[J] & 0xFFFFFFFF) * pinv) & MASK
        Po[J] += MASK - q1
        q2 = ((Po[J] & 0xFFFFFFFF) * pinv) & MASK
        for i in range(S):
            Pe[(i + J) % S] += q1 * pl[i]
            Po[(i + J) % S] += q2 * pl[i]
        tr.see(Pe)
        tr.see(Po)
        assert Pe[J] & MASK == 0 and Po[J] & MASK == 0
        for P in (Pe, Po):
            P[(J + 1) % S] += P[J] >> LB
            P[J] = 0
    return normalize(Pe), normalize(Po)


def pair_mul(A, B, At, Bt, pl, pinv, tr):
    """d4r_run's product: pass A, z = REDC(A_x B_t) on the even lane; pass 1, REDC(A_x A_t) | REDC(B_x A_t - m) + z"""
    z = normalize(lane_pass([0] * S, A, Bt, pl, pinv, tr))
    q1s = []
    Pe = lane_pass([0] * S, A, At, pl, pinv, tr, q1s=q1s)
    Po = lane_pass([0] * S, B, At, pl, pinv, tr, drop=q1s)
    for j in range(S):
        Po[j] += z[j]
    tr.see(Po)
    return normalize(Pe), normalize(Po)


def wide(A, B, pl, tr):
    """c4_wide: u = A + p B over 2 S limbs, limb J retired after row J"""
    P, out = list(A), []
    for J in range(S):
        for i in range(S):
            P[(i + J) % S] += pl[i] * B[J]
        tr.see(P)
        out.append(P[J] & MASK)
        P[(J + 1) % S] += P[J] >> LB
        P[J] = 0
    return out + normalize(P)


# ---------------------------------------------------------------- value level (the same integers)
class Half:
    def __init__(self, p, q):
        assert R >= (1 << 24) * p, "R >= 2^24 p_h"
        self.p, self.q = p, q
        self.pl = limbs(p)
        self.pinvR = pow(p, -1, R)
        self.pinv = (-self.pinvR) % (1 << LB)
        self.x1 = (1 - R) % p
        self.ea = q % (p - 1)
        self.coef = pow(q * q, -1, p * p)

    def redc(self, v):
        """(v + m p) / R and m, the digits of the reduction (m = -v / p mod R)"""
        m = (-v * self.pinvR) % R
        t = v + m * self.p
        assert t % R == 0
        return t // R, m

    def sqr_pair(self, A, B):
        U, m1 = self.redc(A * A)
        Bn, _ = self.redc(self.x1 + 2 * A * B + (R - 1) - m1)
        return U, Bn

    def mul_pair(self, A, B, At, Bt):
        z, _ = self.redc(A * Bt)
        U, m1 = self.redc(A * At)
        w, _ = self.redc(B * At - m1)
        return U, w + z


def sliding_schedule(e, K=5):
    """flexpai.hip sliding_schedule: (first, [(nsq, idx | None), ...])"""
    bit = lambda b: (e >> b) & 1
    i = e.bit_length() - 1

    def window(hi):
        lo = max(hi - K + 1, 0)
        while not bit(lo):
            lo += 1
        v = 0
        for b in range(hi, lo - 1, -1):
            v = (v << 1) | bit(b)
        return lo, v

    lo, v = window(i)
    first = (v - 1) // 2
    i = lo - 1
    ops, nsq = [], 0
    while i >= 0:
        if not bit(i):
            nsq += 1
            i -= 1
            continue
        lo, v = window(i)
        nsq += i - lo + 1
        ops.append((nsq, (v - 1) // 2))
        nsq = 0
        i = lo - 1
    if nsq:
        ops.append((nsq, None))
    return first, ops


SQR, A_FROM_T, STORE, B_CONST, PREFETCH, B_READY, B_SET = 1, 2, 4, 8, 16, 32, 64


def lane_program(e):
    """flexpai.hip build_lane_program: ops as (flags, bidx, aidx, sidx)"""
    assert e.bit_length() >= 8
    first, sched = sliding_schedule(e)
    prog = [[SQR | B_SET, 0, 0, 0], [A_FROM_T | B_READY | STORE, 0, 0, 1]]
    prog += [[STORE | B_READY, 0, 0, k] for k in range(2, 16)]
    loaded, first_sq = False, None
    for nsq, idx in sched:
        for _ in range(nsq):
            if first_sq is None:
                first_sq = len(prog)
            prog.append([SQR, 0, 0, 0] if loaded else [SQR | A_FROM_T, 0, first, 0])
            loaded = True
        if idx is not None:
            if first_sq is not None:
                prog[first_sq][0] |= PREFETCH
                prog[first_sq][1] = idx
                prog.append([B_READY, idx, 0, 0])
            else:
                prog.append([0, idx, 0, 0] if loaded else [A_FROM_T, idx, first, 0])
            loaded = True
            first_sq = None
    assert loaded
    return prog


def mac_count(p, q):
    """lane-MACs per element of the three chains: (stage A, stage B, k_encrypt<8> over the 296 limbs of n^2)"""
    tot = [0, 0]
    for h, (ph, qh) in enumerate(((p, q), (q, p))):
        for st, e in enumerate((qh % (ph - 1), ph)):
            prog = lane_program(e)
            ns = sum(1 for o in prog if o[0] & SQR)
            nm = len(prog) - ns
            if st == 0:
                tot[0] += ns * (S * (S + 1) // 2 + S * S) + nm * 2 * S * S
            else:
                tot[1] += ns * 4 * S * S + (nm + 1) * 8 * S * S
    n = p * q
    first, sched = sliding_schedule(n)
    nops = 16 + sum(nsq + (idx is not None) for nsq, idx in sched) + 2
    return tot[0], tot[1], nops * 2 * 296 * 296


# ---------------------------------------------------------------- one element-half
LIMB_OPS = 3   # ops at the head of each chain that also run on the limb level


def stage_pre(H, r_words, nw, tr):
    """k_crt4_pre: r R mod p from r's words (limb level throughout: K passes)"""
    K = (32 * nw + LB * S - 1) // (LB * S)
    assert 1 <= K <= KMAX_CHUNKS
    cK = pow(R, K + 1, H.p)
    r = sum(w << (32 * i) for i, w in enumerate(r_words[:nw]))
    t = [0] * S
    tv = 0
    for k in range(K):
        dig = [(r >> (LB * (k * S + j))) & MASK for j in range(S)]
        t = normalize(lane_pass(list(t), limbs(cK), dig, H.pl, H.pinv, tr))
        tv, _ = H.redc(tv + cK * val(dig))
        assert val(t) == tv and tv < cK + H.p
    assert tv % H.p == r * R % H.p and tv < 2 * H.p
    return tv


def stage_a(H, x, tr):
    """k_crt4_a: the op list over q mod (p - 1) on one lane, no closing product. Returns y R mod p (< 2p)"""
    p = H.p
    tiles = {0: x}
    a, row = x, None
    for n, (fl, bidx, aidx, sidx) in enumerate(lane_program(H.ea)):
        if fl & A_FROM_T:
            a = tiles[aidx]
        assert a < 2 * p, "operand < 2p"
        if fl & SQR:
            if fl & PREFETCH:
                row = tiles[bidx]
            v, _ = H.redc(a * a)
            if n < LIMB_OPS:
                assert val(lane_sqr(limbs(a), H.pl, H.pinv, tr)) == v
        else:
            if not fl & B_READY:
                row = tiles[bidx]
            v, _ = H.redc(a * row)
            if n < LIMB_OPS:
                assert val(normalize(lane_pass([0] * S, limbs(a), limbs(row), H.pl, H.pinv, tr))) == v
        a = v
        if fl & STORE:
            tiles[sidx] = a
        if fl & B_SET:
            row = a
    assert a < 2 * p
    return a


def stage_b(H, y, tr):
    """k_crt4_b: d4r_run's op list over p from the pair (y, 0), the coefficient's plain pair, the canonical pair, the
    wide product. Returns u (< p^2)"""
    p = H.p
    cA, cB = H.coef % p, H.coef // p
    prog = lane_program(p) + [[B_CONST, 0, 0, 0]]
    tiles = {0: (y, 0)}
    a, st, kept, bclob = (y, 0), None, None, False
    for n, (fl, bidx, aidx, sidx) in enumerate(prog):
        last = n == len(prog) - 1
        if fl & A_FROM_T:
            a = tiles[aidx]
        if fl & SQR and fl & PREFETCH:
            st, bclob = tiles[bidx], False
        assert a[0] < 2 * p and a[1] < 4 * p, "pair operand: A < 2p, B < 4p"
        if fl & SQR:
            v = H.sqr_pair(*a)
            if n < LIMB_OPS:
                lv = pair_sqr(limbs(a[0]), limbs(a[1]), limbs(H.x1), H.pl, H.pinv, tr)
                assert (val(lv[0]), val(lv[1])) == v
            assert v[1] < 2 * p
        else:
            if fl & B_CONST:
                st = (cA, cB)
            elif not fl & B_READY:
                st = tiles[bidx]
            elif bclob:
                st = kept
            v = H.mul_pair(a[0], a[1], st[0], st[1])
            if n < LIMB_OPS or last:
                lv = pair_mul(limbs(a[0]), limbs(a[1]), limbs(st[0]), limbs(st[1]), H.pl, H.pinv, tr)
                assert (val(lv[0]), val(lv[1])) == v
            bclob = True
            assert v[1] < 4 * p, "a product's B < 4p"
        assert v[0] < 2 * p
        a = v
        if fl & STORE:
            tiles[sidx] = a
        if fl & B_SET:
            st, kept, bclob = a, a, False
    A, B = a
    assert (A + p * B) % (p * p) == pow(y * pow(R, -1, p) % p, p, p * p) * H.coef % (p * p), "plain pair of y^p coef"
    # the canonical pair: A >= p moves one p into B, then B < p by at most four subtractions
    if A >= p:
        A, B = A - p, B + 1
    nsub = 0
    while B >= p:
        B -= p
        nsub += 1
    assert nsub <= 4 and A < p
    u = val(wide(limbs(A), limbs(B), H.pl, tr))
    assert u == A + p * B and u < p * p
    return u


def run(p, q, r_words, nw=None):
    """One element: r's little-endian 32-bit words (nw of them, r need not be below n^2) -> r^n mod n^2 through the
    two halves and k_crt_fin's recombination; returns (value, largest accumulator)."""
    nw = len(r_words) if nw is None else nw
    r = sum(w << (32 * i) for i, w in enumerate(r_words[:nw]))
    n = p * q
    tr = Track()
    u = []
    for ph, qh in ((p, q), (q, p)):
        H = Half(ph, qh)
        x = stage_pre(H, r_words, nw, tr)
        y = stage_a(H, x, tr)
        assert y * pow(R, -1, ph) % ph == pow(r, H.ea, ph), "stage A against pow()"
        uh = stage_b(H, y, tr)
        assert uh == pow(r, n, ph * ph) * H.coef % (ph * ph), "stage B against pow()"
        u.append(uh)
    c = (u[0] * q * q + u[1] * p * p) % (n * n)
    assert c == pow(r, n, n * n), "r^n mod n^2"
    return c, tr.mx


def words(r, nw):
    return [(r >> (32 * i)) & 0xFFFFFFFF for i in range(nw)]


def selfcheck(p, q, seed=1, trials=2):
    """limb level == value level for each primitive, on random operands and on operands at their bounds"""
    rng = random.Random(seed)
    H = Half(p, q)
    tr = Track()
    top = lambda k: k * p - 1
    cases = [(rng.randrange(2 * p), rng.randrange(4 * p), rng.randrange(2 * p), rng.randrange(4 * p)) for _ in range(trials)]
    cases += [(top(2), top(4), top(2), top(4)), (0, 0, 0, 0), (top(2), 0, top(2), 0), (1, top(4), p, p)]
    for A, B, At, Bt in cases:
        v, _ = H.redc(A * A)
        assert val(lane_sqr(limbs(A), H.pl, H.pinv, tr)) == v and v < 2 * p
        v, _ = H.redc(A * At)
        assert val(normalize(lane_pass([0] * S, limbs(A), limbs(At), H.pl, H.pinv, tr))) == v and v < 2 * p
        ls = pair_sqr(limbs(A), limbs(B), limbs(H.x1), H.pl, H.pinv, tr)
        vs = H.sqr_pair(A, B)
        assert (val(ls[0]), val(ls[1])) == vs and vs[0] < 2 * p and vs[1] < 2 * p
        Ri = pow(R, -1, p * p)
        assert (vs[0] + p * vs[1]) % (p * p) == (A + p * B) ** 2 * Ri % (p * p)
        lm = pair_mul(limbs(A), limbs(B), limbs(At), limbs(Bt), H.pl, H.pinv, tr)
        vm = H.mul_pair(A, B, At, Bt)
        assert (val(lm[0]), val(lm[1])) == vm and vm[0] < 2 * p and vm[1] < 4 * p
        assert (vm[0] + p * vm[1]) % (p * p) == (A + p * B) * (At + p * Bt) * Ri % (p * p)
    return tr.mx


def is_prime(n, rnd):
    if n < 4:
        return n in (2, 3)
    if n % 2 == 0:
        return False
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for _ in range(8):
        x = pow(rnd.randrange(2, n - 1), d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


_SMALL = [v for v in range(3, 2000, 2) if all(v % d for d in range(3, int(v ** 0.5) + 1, 2))]


def prime_below(v, rnd):
    """the largest prime below v"""
    v -= 1
    if v % 2 == 0:
        v -= 1
    while not (all(v % sp for sp in _SMALL) and is_prime(v, rnd)):
        v -= 2
    return v


def rand_prime(bits, rnd):
    while True:
        v = rnd.getrandbits(bits) | (1 << (bits - 1)) | 1
        if is_prime(v, rnd):
            return v


if __name__ == "__main__":
    rnd = random.Random(4096)
    top = prime_below(1 << 2048, rnd)
    keys = {"2048-bit halves, largest": (prime_below(top, rnd), top),
            "1536-bit halves": (rand_prime(1536, rnd), rand_prime(1536, rnd))}
    for name, (p, q) in keys.items():
        p, q = min(p, q), max(p, q)
        n = p * q
        nw = 2 * ((n.bit_length() + 31) // 32)
        mx = selfcheck(p, q)
        for r in (0, 1, 5 * p, n * n - 1, (1 << (32 * nw)) - 1, rnd.randrange(n * n)):
            _, m = run(p, q, words(r, nw))
            mx = max(mx, m)
        a, b, e8 = mac_count(p, q)
        print(f"{name}: ok, largest accumulator 2^{mx.bit_length()}; lane-MACs per element: stage A {a / 1e6:.1f} M, "
              f"stage B {b / 1e6:.1f} M, k_encrypt<8> {e8 / 1e6:.1f} M, ratio {e8 / (a + b):.2f}")
