"""The limb map PAI_OPT_PRIME_LIMBS = 1 documents (include/flexpai.h), from its inequalities alone: no GPU, no library.

pb: bits of the larger prime of a balanced key (nb = 2 pb), 28-bit limbs. The narrowest sa of (19, 37, 56, 74) with
28 sa >= pb + 12 (the pair bound) whose sb = 2 sa also meets the rows' 28 sb >= 2 pb + 2; kp = ceil(32 W / (28 sa))
ciphertext chunks in the pair decryption above the rows, kd = ceil(32 W / (28 sb)) in k_dec_w, W = ceil(2 nb / 32)."""
import pytest

LB, WIDTHS = 28, (19, 37, 56, 74)
PINNED = {1036: (56, 112, 3, 2), 1536: (56, 112, 4, 2), 1556: (56, 112, 4, 2), 1557: (74, 148, 4, 2)}


def _map(pb):
    sa = next(s for s in WIDTHS if LB * s >= pb + 12 and LB * 2 * s >= 2 * pb + 2)
    W = (2 * 2 * pb + 31) // 32
    return sa, 2 * sa, -(-32 * W // (LB * sa)), -(-32 * W // (LB * 2 * sa))


@pytest.mark.parametrize("pb", range(1035, 1561))
def test_band_map(pb):
    sa, sb, kp, kd = _map(pb)
    assert sa == (56 if pb <= 1556 else 74) and sb == 2 * sa
    assert LB * sa >= pb + 12 > LB * WIDTHS[WIDTHS.index(sa) - 1] and LB * sb >= 2 * pb + 2
    assert kp in (3, 4) and kd == 2          # k_dec4_pre's LDS slot holds 4 chunks of sa limbs
    assert PINNED.get(pb, (sa, sb, kp, kd)) == (sa, sb, kp, kd)
