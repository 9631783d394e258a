"""Key generation's prime search, the parts that need no GPU: the sieve of the device search
(pai_debug_prime_sieve, csrc/engine_prime.hip) against Python trial division by _bigint._SMALL_PRIMES, and the host
path of generate_paillier_keypair ($FLEXPAI_KEYGEN_GPU=0) against the golden keys."""
import os
import random

import pytest


def _native_or_skip():
    from flex.crypto.paillier import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libflexpai.so not built (run __graft_entry__.build())")
    return _native


def _start(bits, seed, odd):
    random.seed(seed)
    x = random.getrandbits(bits) | 1 << (bits - 1)
    return x | 1 if odd else x & ~1


def _trial_division(x, window):
    from flex.crypto.paillier import _bigint
    return [off for off in range(1, window + 1)
            if (x + off) % 2 and all((x + off) % p for p in _bigint._SMALL_PRIMES)]


@pytest.mark.parametrize("window", [64, 4096])
@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("bits", [256, 512, 1024])
def test_sieve_equals_trial_division(bits, odd, window):
    _native = _native_or_skip()
    x = _start(bits, 1000 + bits, odd)
    want = _trial_division(x, window)
    assert _native.prime_sieve(x, bits, window) == want
    assert want and all(0 < off <= window for off in want)


def test_sieve_default_window_and_overflow():
    _native = _native_or_skip()
    x = _start(512, 3, True)
    assert _native.prime_sieve(x, 512) == _trial_division(x, 4 * 512)
    assert _native.prime_sieve((1 << 512) - 1, 512, 64) is None          # the window would cross 2^512
    assert _native.prime_sieve((1 << 512) - 65, 512, 64) == _trial_division((1 << 512) - 65, 64)   # ends at 2^512 - 1
    assert _native.prime_sieve((1 << 512) - 64, 512, 64) is None
    with pytest.raises(_native.NativeError):
        _native.prime_sieve(x, 768, 64)                                  # not a size the kernel is built for
    with pytest.raises(_native.NativeError):
        _native.prime_sieve(x >> 1, 512, 64)                             # bit 511 not set


def test_host_fallback_gives_the_golden_key(golden, monkeypatch):
    from flex.crypto.paillier import _bigint, _native
    from flex.crypto.paillier.keypair import generate_paillier_keypair
    monkeypatch.setenv("FLEXPAI_KEYGEN_GPU", "0")
    assert not _bigint.keygen_on_device(512)
    rec = next(r for r in golden["keygen"] if (r["nb"], r["seed"]) == (1024, 1))
    before = _native.prime_stats()
    pk, sk = generate_paillier_keypair(1024, seed=1)
    assert (hex(pk.n), hex(sk.p), hex(sk.q)) == (rec["n"], rec["p"], rec["q"])
    assert _native.prime_stats() == before                               # no device search, no counted fallback
    # the state of the random module afterwards: q's draw was the last one
    random.seed(2)
    random.getrandbits(512)
    want = random.getstate()
    generate_paillier_keypair(1024, seed=1)
    assert random.getstate() == want
