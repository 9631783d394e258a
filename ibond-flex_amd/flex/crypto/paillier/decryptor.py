"""PaillierDecryptor — same API and errors as flex/crypto/paillier/decryptor.py:28-127.

Arrays decrypt in ONE device call: both CRT half-exponentiations c^(p-1) mod p^2 and c^(q-1) mod q^2,
the L-function, the CRT recombination and the fixed-point decode to float64 run on the GPU -- the
lane-engine kernels k_dec_pre / k_dec_pow / k_dec_fin (kernels_dec.hpp) for 1024- and 2048-bit keys,
the lane-group kernel k_decrypt (kernels.hpp) for larger ones. A CiphertextBuffer (cipher_buffer.py)
decrypts straight from its words, without per-element objects."""
from __future__ import annotations

from typing import Union

import numpy as np

from .encrypted_number import PaillierEncryptedNumber
from .fixedpoint_number import FixedPointNumber
from .keypair import PaillierPrivateKey, PaillierPublicKey


class PaillierDecryptor(object):
    def __init__(self, pub_key: PaillierPublicKey, priv_key: PaillierPrivateKey):
        self.pub_key = pub_key
        self.priv_key = priv_key
        from . import _runtime
        _runtime.register_private(pub_key, priv_key)

    def __setstate__(self, state):
        # unpickled in another process (the reference pickles decryptors into pool workers)
        self.__dict__.update(state)
        from . import _runtime
        _runtime.register_private(self.pub_key, self.priv_key)

    def _check(self, encrypted_number):
        if not isinstance(encrypted_number, PaillierEncryptedNumber):          # decryptor.py:73-75
            raise TypeError("encrypted_number should be an PaillierEncryptedNumber, \
                             not: %s" % type(encrypted_number))
        if self.pub_key != encrypted_number.public_key:                        # decryptor.py:77-79
            raise ValueError("encrypted_number was encrypted against a different key!")

    def _decrypt(self, encrypted_number: PaillierEncryptedNumber) -> Union[int, float]:
        """decryptor.py:65-89"""
        self._check(encrypted_number)
        out = np.array([encrypted_number], dtype=object)
        v = self._decrypt_numpy(out).reshape(-1)[0]
        return v.item() if isinstance(v, np.generic) else v

    def _decrypt_numpy(self, encrypted_number_numpy: np.ndarray) -> np.ndarray:
        """decryptor.py:91-112, one batched GPU launch. The per-element _check and the packing of the
        ciphertexts run as one C pass (cipher_array.pack_checked; a PaillierArray whose packed words are
        still valid only checks); the reference's exceptions come from the per-element path when it fails."""
        from .cipher_array import PaillierArray, pack, pack_checked
        s = encrypted_number_numpy.shape
        flat = np.asarray(encrypted_number_numpy).reshape(-1)
        if flat.size == 0:
            return np.array([]).reshape(s)
        W = (2 * self.pub_key.n.bit_length() + 31) // 32
        cached = encrypted_number_numpy._valid_packed() if isinstance(encrypted_number_numpy, PaillierArray) else None
        if cached is not None and cached.n == self.pub_key.n:
            if pack_checked(flat, self.pub_key, W, want_words=False) is not None:
                return self._decrypt_words(cached.words, cached.exps.astype(np.int32), s)
        else:
            got = pack_checked(flat, self.pub_key, W)
            if got is not None:
                return self._decrypt_words(got[0], got[1], s)
        for e in flat:
            self._check(e)
        words, exps, _ = pack(encrypted_number_numpy, self.pub_key)
        return self._decrypt_words(words, exps, s)

    def _decrypt_words(self, words, exps, s) -> np.ndarray:
        """words: numpy [N, W], or a device holder (device_buffer.DeviceWords) with the exponents as a device block: then
        pai_decrypt_dev runs where the words are, and only values and statuses come back."""
        from . import _native, _runtime
        if isinstance(words, np.ndarray):
            ctx = _runtime.context(self.pub_key, self.priv_key)
            run = lambda want_raw=False: ctx.decrypt(words, exps, want_raw=want_raw)          # noqa: E731
        else:
            from .device_buffer import decrypt_dev
            run = lambda want_raw=False: decrypt_dev(self.pub_key, self.priv_key, words, exps, want_raw)   # noqa: E731
        val, mant, st, _ = run()
        if np.all(st == _native.EL_OK):
            return val.reshape(s)
        for code, exc, msg in ((_native.EL_OVERFLOW, OverflowError, 'Overflow detected in decode number'),
                               (_native.EL_FLOAT_OVF, OverflowError, 'int too large to convert to float')):
            if np.any(st == code):
                raise exc(msg)
        raw = None
        if np.any(st == _native.EL_INT_BIG):
            _, _, _, raw_words = run(True)
            raw = _runtime.words_to_ints(raw_words)
        ex = exps if isinstance(exps, np.ndarray) else exps.download(np.int32, st.size)
        values = []
        for i in range(ex.size):
            if st[i] == _native.EL_OK:
                values.append(float(val[i]))
            elif st[i] == _native.EL_INT:
                values.append(int(mant[i]))
            else:   # exact integer too wide for int64: decode the exact plaintext
                values.append(FixedPointNumber(raw[i], int(ex[i]), self.pub_key.n, self.pub_key.max_int).decode())
        return np.array(values).reshape(s)

    def _decrypt_packed(self, buf) -> np.ndarray:
        """A PackedCiphertextBuffer (packed_buffer.py) in ONE pai_decrypt_packed call: float64 values of buf.shape,
        int64 when the layout's exponent is 0."""
        from . import _native, _runtime
        from .packed_buffer import host_decrypt_packed
        if buf.public_key != self.pub_key:
            raise ValueError("encrypted_number was encrypted against a different key!")
        e = buf.layout.exponent
        if buf.count == 0:
            return np.zeros(buf.shape, dtype=np.int64 if e == 0 else np.float64)
        if buf.resident:
            from .device_buffer import decrypt_packed_dev
            val, mant, st = decrypt_packed_dev(self.pub_key, self.priv_key, buf.words, buf.layout, buf.count)
            if np.any(st == _native.EL_OVERFLOW):
                raise OverflowError('Overflow detected in decode number')
        elif _runtime.gpu_available():
            val, mant, st = _runtime.context(self.pub_key, self.priv_key).decrypt_packed(buf.words, buf.layout, buf.count)
            if np.any(st == _native.EL_OVERFLOW):
                raise OverflowError('Overflow detected in decode number')
        else:
            mant = np.array(host_decrypt_packed(buf, self.priv_key), dtype=np.int64)
            val = np.ldexp(mant.astype(np.float64), -4 * e)
        return (mant if e == 0 else val).reshape(buf.shape)

    def decrypt(self, encrypted_number):
        """decryptor.py:114-127 (plus CiphertextBuffer, cipher_buffer.py, DeviceCiphertextBuffer, device_buffer.py, and
        PackedCiphertextBuffer, host or resident)"""
        from .cipher_buffer import CiphertextBuffer
        from .device_buffer import DeviceCiphertextBuffer
        from .packed_buffer import PackedCiphertextBuffer
        if isinstance(encrypted_number, PackedCiphertextBuffer):
            return self._decrypt_packed(encrypted_number)
        if isinstance(encrypted_number, DeviceCiphertextBuffer):
            if encrypted_number.public_key != self.pub_key:
                raise ValueError("encrypted_number was encrypted against a different key!")
            if encrypted_number.size == 0:
                return np.array([]).reshape(encrypted_number.shape)
            return self._decrypt_words(encrypted_number.words, encrypted_number._ex, encrypted_number.shape)
        if isinstance(encrypted_number, CiphertextBuffer):
            if encrypted_number.public_key != self.pub_key:
                raise ValueError("encrypted_number was encrypted against a different key!")
            if encrypted_number.size == 0:
                return np.array([]).reshape(encrypted_number.shape)
            return self._decrypt_words(encrypted_number.words, encrypted_number.exps, encrypted_number.shape)
        if isinstance(encrypted_number, np.ndarray):
            return self._decrypt_numpy(encrypted_number)
        return self._decrypt(encrypted_number)
