"""apply_obfuscation — same signature as flex/crypto/paillier/obfuscator.py:23-37.

c * r^n mod n^2. The modular exponentiation r^n mod n^2 (~99 % of the reference's encryption
time) runs on the GPU: it is the device encryption of the integer 0 (c0 = 1) with obfuscator r
(given) or with a fresh device-CSPRNG r (random_value None)."""
import numpy as np

from . import _bigint as gmpy_math


def obfuscator_power(pub_key, random_value: int = None) -> int:
    """r^n mod n^2 computed on the GPU; with random_value None and obfuscators prepared ahead of time
    (obfuscator_pool.prepare_obfuscators), the next one of the pool instead of an exponentiation."""
    from . import _native, _runtime, obfuscator_pool
    if not random_value:
        with obfuscator_pool.lock:
            taken = obfuscator_pool.host_pool_take(pub_key, 1)
            if taken:
                return taken[0]
            ctx = obfuscator_pool.device_pool(pub_key, 1)
            if ctx is not None:
                ct, _, _ = ctx.encrypt(np.zeros(1, dtype=np.int64), obf_mode=_native.PAI_OBF_POOL)
                return _native.words_to_ints(ct)[0]
    ctx = _runtime.context(pub_key)
    zero = np.zeros(1, dtype=np.int64)
    if random_value:
        ct, _, _ = ctx.encrypt(zero, obf_mode=_native.PAI_OBF_GIVEN, r_scalar=int(random_value) % pub_key.nsquare)
    else:
        ct, _, _ = ctx.encrypt(zero, obf_mode=_native.PAI_OBF_RNG)
    return _native.words_to_ints(ct)[0]


def apply_obfuscation_array(words, pub_key, random_value: int = None) -> np.ndarray:
    """The array twin of apply_obfuscation: [N, W] little-endian uint32 ciphertext words -> the words of
    c_i * r_i^n mod n^2, in ONE GPU call (pai_obfuscate: r^n by the encrypt chains, one product kernel). random_value
    None (or 0, as in obfuscator_power): a fresh device-CSPRNG r per element; an int: that r for every element, reduced
    mod n^2 as PaillierEncryptor._encrypt_numpy reduces it; 1: a copy (mulmod(c, 1, n^2))."""
    from . import _native, _runtime, obfuscator_pool
    words = np.ascontiguousarray(words, dtype=np.uint32)
    if random_value == 1:
        return words.copy()
    if not random_value:                     # obfuscators prepared ahead of time, when they cover the whole array
        with obfuscator_pool.lock:
            taken = obfuscator_pool.host_pool_take(pub_key, words.shape[0])
            if taken:
                nsq = pub_key.nsquare
                cs = _native.words_to_ints(words)
                return _native.ints_to_words([gmpy_math.mulmod(c, s, nsq) for c, s in zip(cs, taken)], words.shape[1])
            ctx = obfuscator_pool.device_pool(pub_key, words.shape[0])
            if ctx is not None:
                return ctx.obfuscate(words, obf_mode=_native.PAI_OBF_POOL)
    ctx = _runtime.context(pub_key)
    if random_value:
        return ctx.obfuscate(words, obf_mode=_native.PAI_OBF_GIVEN, r_scalar=int(random_value) % pub_key.nsquare)
    return ctx.obfuscate(words, obf_mode=_native.PAI_OBF_RNG)


def apply_obfuscation(ciphertext: int, pub_key, random_value: int = None) -> int:
    if random_value == 1:
        return gmpy_math.mulmod(ciphertext, 1, pub_key.nsquare)     # gmpy_math.powmod(1, ...) == 1
    obfuscator = obfuscator_power(pub_key, random_value)
    return gmpy_math.mulmod(ciphertext, obfuscator, pub_key.nsquare)
