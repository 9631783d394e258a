"""Key generation on the GPU (csrc/kernels_prime.hpp k_mr_w, csrc/engine_prime.hip): the verdict matrix of the
strong-probable-prime test against the host's per-base test, pai_next_prime against _bigint.next_prime, and
generate_paillier_keypair on the device path against the golden keys with the host's primality test disabled. The
candidates here are random primes, golden primes and their products; moduli, exponents of two, bases, pseudoprimes and
starts at the edges of the kernel's arithmetic are in test_gpu_prime_edges.py."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bases():
    from flex.crypto.paillier import _bigint
    return _bigint._SMALL_PRIMES[:40]


def _strong_test(n, a):
    """_bigint.is_probable_prime's inner loop for one base; returns (verdict, exit taken)."""
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    y = pow(a, d, n)
    if y == 1:
        return True, "one"
    if y == n - 1:
        return True, "minus_one"
    for _ in range(s - 1):
        y = y * y % n
        if y == n - 1:
            return True, "squared"
    return False, "never"


def _rec(golden, nb, seed):
    r = next(r for r in golden["keygen"] if (r["nb"], r["seed"]) == (nb, seed))
    return int(r["p"], 16), int(r["q"], 16), int(r["n"], 16)


def _built_prime(bits, residue, modulus, seed):
    """A `bits`-bit prime == residue mod modulus, by the host functions."""
    from flex.crypto.paillier import _bigint
    rng = random.Random(seed)
    while True:
        c = rng.getrandbits(bits) | 1 << (bits - 1)
        c = c - c % modulus + residue
        if c.bit_length() == bits and _bigint.is_probable_prime(c):
            return c


@pytest.fixture(scope="module")
def candidates(golden):
    from flex.crypto.paillier import _bigint
    p512, q512, n512 = _rec(golden, 512, 99)
    p1k, _, n1k = _rec(golden, 1024, 1)
    _, _, n1k2 = _rec(golden, 1024, 2)
    p2k, q2k, n2k = _rec(golden, 2048, 1)
    p4k, _, _ = _rec(golden, 4096, 7)
    random.seed(77)
    a128 = _bigint.next_prime(random.getrandbits(128) | 3 << 126)
    b128 = _bigint.next_prime(random.getrandbits(128) | 3 << 126)
    assert (a128 * b128).bit_length() == 256
    return {
        256: [p512, q512, _built_prime(256, 1, 64, 1), _built_prime(256, 3, 4, 2), a128 * b128],
        512: [p1k, _built_prime(512, 1, 64, 3), n512],
        1024: [p2k, q2k, n1k, n1k2],
        2048: [p4k, n2k],
    }


@pytest.fixture(scope="module")
def host_matrix(candidates):
    """The host's verdict and exit for every (candidate, base), computed once."""
    return {bits: [[_strong_test(n, a) for a in _bases()] for n in cs] for bits, cs in candidates.items()}


def test_candidates_cover_every_exit(host_matrix):
    exits = {e for rows in host_matrix.values() for row in rows for _, e in row}
    assert exits == {"one", "minus_one", "squared", "never"}


@pytest.mark.parametrize("bits", [256, 512, 1024, 2048])
def test_verdict_matrix_equals_host(bits, candidates, host_matrix):
    from flex.crypto.paillier import _native
    got = _native.prime_test(candidates[bits], bits, _bases())
    want = np.array([[v for v, _ in row] for row in host_matrix[bits]], dtype=np.uint8)
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("nwork", [1, 5, 67])
def test_ragged_work_counts(nwork, candidates, host_matrix):
    """Work counts that do not fill a wave's four rows, and more than one block."""
    from flex.crypto.paillier import _native
    cs, rows = candidates[256], host_matrix[256]
    if nwork == 1:
        got = _native.prime_test(cs[4:5], 256, _bases()[7:8])
        assert got.tolist() == [[int(rows[4][7][0])]]
    elif nwork == 5:
        got = _native.prime_test(cs, 256, _bases()[:1])
        assert got[:, 0].tolist() == [int(r[0][0]) for r in rows]
    else:
        got = _native.prime_test(cs[2:3], 256, _bases() + _bases()[:27])
        want = [int(v) for v, _ in rows[2]]
        assert got[0].tolist() == want + want[:27]


def _seeded_start(bits, seed):
    random.seed(seed)
    return random.getrandbits(bits) | 1 << (bits - 1)


@pytest.mark.parametrize("bits,seeds", [(256, (11, 12, 13)), (512, (21, 22, 23)), (1024, (31, 32, 33)), (2048, (41,))])
def test_next_prime_equals_host(bits, seeds):
    from flex.crypto.paillier import _bigint, _native
    starts = [_seeded_start(bits, s) for s in seeds]
    primes, passes = _native.next_prime_batch(starts, bits)
    assert primes == [_bigint.next_prime(x) for x in starts]
    assert all(k >= 1 for k in passes)


def test_next_prime_is_strictly_greater(golden):
    from flex.crypto.paillier import _native
    p, q, _ = _rec(golden, 1024, 1)
    primes, _ = _native.next_prime_batch([p - 2, p - 1, p], 512)
    assert primes[0] == p and primes[1] == p
    assert primes[2] > p and primes[2] == _native.next_prime_batch([p + 1], 512)[0][0]


def test_window_advance_small_window():
    """A gap of 400 with 31 sieve survivors before the prime: with 64-wide windows the search moves on several times."""
    from flex.crypto.paillier import _bigint, _native
    x = _seeded_start(512, 5)
    want = _bigint.next_prime(x)
    assert want - x == 400
    primes, passes = _native.next_prime_batch([x], 512, window=64)
    assert primes == [want] and passes == [7]                  # ceil(400 / 64)
    assert _native.next_prime_batch([x], 512)[0] == [want]


def test_long_gap_at_the_default_window():
    """A gap of 1932 with 139 sieve survivors before the prime, at 1024 bits."""
    from flex.crypto.paillier import _bigint, _native
    x = _seeded_start(1024, 2)
    want = _bigint.next_prime(x)
    assert want - x == 1932
    primes, passes = _native.next_prime_batch([x], 1024)
    assert primes == [want] and passes == [1]                  # the default window, 4096, holds it


def test_batch_equals_single_calls():
    from flex.crypto.paillier import _native
    starts = [_seeded_start(512, s) for s in (51, 52, 53, 54)]
    batch, _ = _native.next_prime_batch(starts, 512)
    assert batch == [_native.next_prime_batch([x], 512)[0][0] for x in starts]


def test_overflow_start_is_handed_back():
    from flex.crypto.paillier import _bigint, _native
    x = _seeded_start(256, 61)
    primes, passes = _native.next_prime_batch([(1 << 256) - 3, x], 256)
    assert primes[0] is None and passes[0] == -1
    assert primes[1] == _bigint.next_prime(x) and passes[1] >= 1


@pytest.mark.parametrize("nb,seed", [(1024, 1), (1024, 2), (1024, 12345), (2048, 1), (4096, 7), (512, 99)])
def test_keygen_on_device_gives_the_golden_key(nb, seed, golden, monkeypatch):
    from flex.crypto.paillier import _bigint, _native
    from flex.crypto.paillier.keypair import generate_paillier_keypair
    monkeypatch.delenv("FLEXPAI_KEYGEN_GPU", raising=False)
    p, q, n = _rec(golden, nb, seed)

    def no_host_test(x):
        raise AssertionError("the host's primality test ran: the search fell back silently")

    before = _native.prime_stats()
    with monkeypatch.context() as m:
        m.setattr(_bigint, "is_probable_prime", no_host_test)
        pk, sk = generate_paillier_keypair(nb, seed=seed)
        state = random.getstate()
    after = _native.prime_stats()
    assert (pk.n, sk.p, sk.q) == (n, p, q)
    assert after["device_searches"] >= before["device_searches"] + 2
    assert after["host_fallbacks"] == before["host_fallbacks"]
    if nb <= 1024:
        monkeypatch.setenv("FLEXPAI_KEYGEN_GPU", "0")
        hk, hs = generate_paillier_keypair(nb, seed=seed)
        assert (hk.n, hs.p, hs.q) == (n, p, q) and random.getstate() == state
        assert _native.prime_stats() == after


def test_device_key_round_trip(monkeypatch):
    from flex.crypto.paillier import _native
    from flex.crypto.paillier.keypair import generate_paillier_keypair
    monkeypatch.delenv("FLEXPAI_KEYGEN_GPU", raising=False)
    before = _native.prime_stats()["device_searches"]
    pk, sk = generate_paillier_keypair(1024, seed=4711)
    assert _native.prime_stats()["device_searches"] >= before + 2 and pk.n.bit_length() == 1024
    ctx = _native.Context(pk.n, 0, sk.p, sk.q)
    x = np.linspace(-3.75, 3.75, 16).astype(np.float64)        # halves' multiples, none an integer: status PAI_EL_OK
    ct, ex, st = ctx.encrypt(x, rng_key=bytes(range(32)), index_base=0)
    assert not np.asarray(st).any()
    val, _, st2, _ = ctx.decrypt(ct, ex)
    assert not np.asarray(st2).any() and np.array_equal(np.asarray(val, dtype=np.float64), x)
