"""The encrypt route (csrc/encrypt_route.hpp) as a table: which fixed-base sampler a call is eligible for and which
per-element kernels it runs on otherwise, for each kind of context, through pai_debug_encrypt_route. The hook is a pure
function of the facts it is given, so this needs the built library but no device.

For an explicit r every chain gives the same ciphertext bits, so the parity tests cannot see a wrong route; the GPU
suites probe single thresholds through stage counts. This pins the order as a whole."""
import ctypes
import os

import pytest

from flex.crypto.paillier import _native

NONE, GIVEN, RNG = _native.PAI_OBF_NONE, _native.PAI_OBF_GIVEN, _native.PAI_OBF_RNG
S_NONE, S_KEY, S_PUBLIC = 0, 1, 2
ENCRYPT, CRT_ROWS, CRT_ROWS4, CRT_LANE, CRT4, PE_ROWS, PE, PE1, PE4 = range(9)


class Facts(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in (
        "has_priv", "crt_enabled", "fb_enabled", "pfb_enabled", "crt_ok", "crt_sa", "fbg_ok", "rows_sa", "crt4_ok",
        "pe_ok", "pe1_ok", "pe4_ok", "pew_ok", "pfb_supported", "ct_words", "rows_r_max")] + [
        ("crtw_max", ctypes.c_longlong), ("crt4_min", ctypes.c_longlong)]


def test_header_and_binding_agree_on_the_constants():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "flexpai.h")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (PAI_(?:SAMPLER|CHAIN)_\w+) (\d+)", hdr)}
    assert [val["PAI_SAMPLER_" + k] for k in ("NONE", "KEY", "PUBLIC")] == [S_NONE, S_KEY, S_PUBLIC]
    assert [val["PAI_CHAIN_" + k] for k in ("ENCRYPT", "CRT_ROWS", "CRT_ROWS4", "CRT_LANE", "CRT4", "PE_ROWS", "PE", "PE1",
                                            "PE4")] == list(range(9))
    body = re.search(r"typedef struct pai_route_facts \{(.*?)\} pai_route_facts;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(long long|int)\s", "", decl.strip()).split(",")]
    assert names == [k for k, _ in Facts._fields_]


# a context's facts at the defaults (ROWS_MAX 4096, CRT4_MIN 128); every context has the k_pe_w op list
BASE = dict(crt_enabled=1, fb_enabled=1, pfb_enabled=1, pew_ok=1, crtw_max=4096, crt4_min=128)
KEY1024 = dict(BASE, has_priv=1, crt_ok=1, crt_sa=19, pe1_ok=1, ct_words=64)
KEY2048 = dict(BASE, has_priv=1, crt_ok=1, crt_sa=37, pe_ok=1, pfb_supported=1, ct_words=128)
KEY4096 = dict(BASE, has_priv=1, fbg_ok=1, rows_sa=74, crt4_ok=1, pe4_ok=1, ct_words=256, rows_r_max=256)
PUB1024 = dict(BASE, pe1_ok=1, ct_words=64)
PUB2048 = dict(BASE, pe_ok=1, pfb_supported=1, ct_words=128)
PUB4096 = dict(BASE, pe4_ok=1, ct_words=256)
RW = {64: 34, 128: 66, 256: 130}   # words of the device-RNG stream of r: (key bits + 64 + 31) / 32

# (facts, overrides, obf, n, r_words or None for the usual width) -> (sampler, chain)
TABLE = [
    # key holder, 1024 / 2048 bits: rows up to ROWS_MAX, lane CRT above; device RNG adds the key holder's sampler
    *[(k, {}, GIVEN, 4096, None, S_NONE, CRT_ROWS) for k in (KEY1024, KEY2048)],
    *[(k, {}, GIVEN, 4097, None, S_NONE, CRT_LANE) for k in (KEY1024, KEY2048)],
    *[(k, {}, RNG, 4096, None, S_KEY, CRT_ROWS) for k in (KEY1024, KEY2048)],
    *[(k, {}, RNG, 4097, None, S_KEY, CRT_LANE) for k in (KEY1024, KEY2048)],
    *[(k, dict(fb_enabled=0), RNG, n, None, S_NONE, ch) for k in (KEY1024, KEY2048)
      for n, ch in ((4096, CRT_ROWS), (4097, CRT_LANE))],
    # an over-wide r is not the route's business at these sizes: launch_crt rejects it
    (KEY2048, {}, GIVEN, 100, 128, S_NONE, CRT_ROWS),
    # ... with the CRT switched off they are public-key parties
    (KEY2048, dict(crt_enabled=0), RNG, 4096, None, S_PUBLIC, PE_ROWS),
    (KEY2048, dict(crt_enabled=0), RNG, 4097, None, S_PUBLIC, PE),
    (KEY2048, dict(crt_enabled=0), GIVEN, 4096, None, S_NONE, PE_ROWS),
    (KEY2048, dict(crt_enabled=0), GIVEN, 4097, None, S_NONE, PE),
    (KEY1024, dict(crt_enabled=0), RNG, 4096, None, S_NONE, PE_ROWS),
    (KEY1024, dict(crt_enabled=0), RNG, 4097, None, S_NONE, PE1),
    # key holder, 4096 bits
    (KEY4096, {}, GIVEN, 4096, None, S_NONE, CRT_ROWS4),
    (KEY4096, {}, GIVEN, 4097, None, S_NONE, CRT4),
    (KEY4096, {}, RNG, 4096, None, S_KEY, CRT_ROWS4),
    (KEY4096, {}, RNG, 4097, None, S_KEY, CRT4),
    (KEY4096, dict(fb_enabled=0), RNG, 4096, None, S_NONE, CRT_ROWS4),
    (KEY4096, dict(crtw_max=0), GIVEN, 128, None, S_NONE, ENCRYPT),     # k_pe4_* never with a private key
    (KEY4096, dict(crtw_max=0), GIVEN, 129, None, S_NONE, CRT4),
    (KEY4096, dict(crtw_max=0), RNG, 128, None, S_KEY, ENCRYPT),
    (KEY4096, dict(crtw_max=0, crt4_min=0), GIVEN, 1, None, S_NONE, CRT4),
    (KEY4096, {}, GIVEN, 4096, 256, S_NONE, CRT_ROWS4),                  # the widest r the rows stage
    (KEY4096, {}, GIVEN, 4096, 257, S_NONE, CRT4),                       # wider: skips the rows, goes on down
    (KEY4096, {}, GIVEN, 128, 257, S_NONE, PE_ROWS),
    (KEY4096, dict(crt_enabled=0), GIVEN, 4096, None, S_NONE, PE_ROWS),
    (KEY4096, dict(crt_enabled=0), RNG, 4097, None, S_NONE, ENCRYPT),
    # public key only
    (PUB2048, {}, RNG, 4096, None, S_PUBLIC, PE_ROWS),                   # the sampler ahead of the rows
    (PUB2048, {}, RNG, 4097, None, S_PUBLIC, PE),
    (PUB2048, {}, GIVEN, 4096, None, S_NONE, PE_ROWS),
    (PUB2048, {}, GIVEN, 4097, None, S_NONE, PE),
    (PUB2048, dict(pfb_enabled=0), RNG, 4096, None, S_NONE, PE_ROWS),
    (PUB2048, dict(pfb_enabled=0), RNG, 4097, None, S_NONE, PE),
    (PUB2048, dict(crtw_max=0), GIVEN, 1, None, S_NONE, PE),
    *[(PUB4096, {}, obf, 4096, None, S_NONE, PE_ROWS) for obf in (GIVEN, RNG)],
    *[(PUB4096, {}, obf, 4097, None, S_NONE, PE4) for obf in (GIVEN, RNG)],
    *[(PUB1024, {}, obf, 4096, None, S_NONE, PE_ROWS) for obf in (GIVEN, RNG)],
    *[(PUB1024, {}, obf, 4097, None, S_NONE, PE1) for obf in (GIVEN, RNG)],
    # no obfuscation: k_encrypt in every context
    *[(k, {}, NONE, n, 0, S_NONE, ENCRYPT) for k in (KEY1024, KEY2048, KEY4096, PUB1024, PUB2048, PUB4096)
      for n in (1, 4096, 4097)],
]


def test_encrypt_route_table():
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libflexpai.so not built (run __graft_entry__.build())")
    lib = _native.load_library()
    for row, (facts, over, obf, n, rw, sampler, chain) in enumerate(TABLE):
        f = Facts(**dict(facts, **over))
        s, ch = ctypes.c_int(-1), ctypes.c_int(-1)
        rw = RW[f.ct_words] if rw is None else rw
        assert lib.pai_debug_encrypt_route(ctypes.byref(f), obf, n, rw, ctypes.byref(s), ctypes.byref(ch)) == 0
        assert (s.value, ch.value) == (sampler, chain), (row, dict(facts, **over), obf, n, rw)
    assert lib.pai_debug_encrypt_route(None, GIVEN, 1, 1, None, None) != 0
