"""The broadcast multiply without a GPU: the axis rule of cipher_array.bcast_row_form against numpy's own broadcasting
on index arrays, and the new names and numbers of the C ABI."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("a_shape,x_shape", [((6,), (4, 6)), ((6, 1), (6, 5)), ((1, 6), (4, 6)), ((3, 1, 2), (3, 4, 2)),
                                             ((2, 1, 3, 1), (5, 2, 4, 3, 7)), ((), (2, 3)), ((4, 1), (3,))])
def test_axis_rule(a_shape, x_shape):
    """Row i of x2d holds the scalars that ciphertext i meets, and argsort(perm) puts the [N, F] outputs in numpy's
    order: checked with position arrays in place of ciphertexts and scalars."""
    from flex.crypto.paillier.cipher_array import bcast_row_form
    ia = np.arange(int(np.prod(a_shape)), dtype=np.int64).reshape(a_shape)
    ix = np.arange(int(np.prod(x_shape)), dtype=np.int64).reshape(x_shape)
    x2d, shape, perm = bcast_row_form(a_shape, ix)
    wa, wx = np.broadcast_arrays(ia, ix)
    assert shape == wa.shape and x2d.shape == (ia.size, wa.size // ia.size)
    rows = np.repeat(np.arange(ia.size), x2d.shape[1]).reshape([shape[k] for k in perm]).transpose(np.argsort(perm))
    assert np.array_equal(rows, wa)
    assert np.array_equal(x2d.reshape([shape[k] for k in perm]).transpose(np.argsort(perm)), wx)


def test_axis_rule_leaves_other_calls_alone():
    from flex.crypto.paillier.cipher_array import bcast_row_form
    assert bcast_row_form((4, 6), np.zeros(6)) is None and bcast_row_form((4, 6), np.zeros((4, 6))) is None
    with pytest.raises(ValueError):
        bcast_row_form((6,), np.zeros((4, 5)))


def test_buffer_without_a_gpu_runs_on_python_integers(monkeypatch):
    """CiphertextBuffer(3,) * X(2, 3) with no GPU: the per-element operator's bits in the broadcast shape (the permuted
    case); an empty plain array of another shape keeps raising."""
    import json
    from flex.crypto.paillier import _runtime
    from flex.crypto.paillier.cipher_buffer import CiphertextBuffer
    from flex.crypto.paillier.encrypted_number import PaillierEncryptedNumber
    from flex.crypto.paillier.keypair import PaillierPublicKey
    monkeypatch.setattr(_runtime, "gpu_available", lambda: False)
    with open(os.path.join(ROOT, "tests", "golden", "paillier_golden.json")) as f:
        pk = PaillierPublicKey(int(json.load(f)["keys"]["1024"]["n"], 16))
    cs, es = [pow(7, 1000 + i, pk.nsquare) for i in range(3)], [3, -2, 0]
    buf = CiphertextBuffer(pk, _runtime.ints_to_words(cs, (2 * pk.n.bit_length() + 31) // 32), es)
    X = np.array([[1.5, -2.0, 0.0], [3.0, 0.25, -7.0]])
    got = (buf * X).to_array()
    assert got.shape == (2, 3)
    for r in range(2):
        for i in range(3):
            want = PaillierEncryptedNumber(pk, cs[i], es[i]) * float(X[r, i])
            assert (got[r, i].ciphertext(False), got[r, i].exponent) == (want.ciphertext(False), want.exponent)
    with pytest.raises((TypeError, ValueError, RuntimeError)):
        buf * np.zeros((0, 3))


def test_names_and_numbers():
    from flex.crypto.paillier import _native
    header = open(os.path.join(ROOT, "include", "flexpai.h")).read()
    numbers = dict(re.findall(r"^#define (PAI_OPT_MUL_BCAST\w*) (\d+)", header, re.M))
    assert numbers == {"PAI_OPT_MUL_BCAST": "29", "PAI_OPT_MUL_BCAST_PATH": "30"}
    assert (_native.PAI_OPT_MUL_BCAST, _native.PAI_OPT_MUL_BCAST_PATH) == (29, 30)
    assert {"pai_mul_bcast", "pai_mul_bcast_dev"} <= set(_native.EXPORTED)
