"""Obfuscators drawn ahead of time (no reference counterpart: the reference draws r and computes r^n mod n^2 inside every
encrypt, obfuscator.py:23-37).

r^n does not depend on the plaintext. A party that waits for its peer calls prepare_obfuscators(pub_key, count); the
encryptions and re-randomisations that follow spend one ready obfuscator per fresh ciphertext, (1 + n m) rho mod n^2,
instead of one exponentiation. With a GPU the pool is the ring of the process's native context (include/flexpai.h,
"Obfuscator pool": filled by the party's ordinary encryption route, so pooled ciphertexts have the distribution of its
ordinary ones); without one it is a list of Python ints. It lives with the per-process context: it is never pickled and
never on the wire, and a context dropped from the cache (_runtime: $FLEXPAI_MAX_CONTEXTS) takes its pool with it.

Every entry is used exactly once: two ciphertexts under one obfuscator reveal the difference of their plaintexts
("Obfuscator keys"). A call is served from the pool only when a pool was prepared AND holds the whole
call's count; otherwise the unchanged route runs and the pool is untouched. A process that never calls
prepare_obfuscators makes exactly the calls it made before.
"""
from __future__ import annotations

import collections
import os
import secrets
import threading
import weakref
from typing import Dict, List, Tuple

from . import _bigint as gmpy_math

DEFAULT_CHUNK = 65536

# taken around "does the pool hold the call's count" and the call that spends it, so that two threads of one process
# cannot both be promised the same entries (the native ring would refuse the second, which would then fail, not fall back)
lock = threading.RLock()
_device: Dict[Tuple[int, int, int], "weakref.ref"] = {}             # (n, device, pid) -> the context whose ring was prepared
_host: Dict[Tuple[int, int], "collections.deque[int]"] = {}          # (n, pid) -> ready r^n mod n^2, oldest first


def _gpu() -> bool:
    from . import _runtime
    return _runtime.gpu_available()


def _device_ctx(pub_key):
    """The context whose ring this process prepared for pub_key, if it is still the cached one."""
    from . import _runtime
    k = (pub_key.n, _runtime.device_index(), os.getpid())
    ref = _device.get(k)
    if ref is None:
        return None
    ctx = ref()
    if ctx is None or ctx is not _runtime.context(pub_key):
        _device.pop(k, None)                                          # evicted with its pool: back to the ordinary routes
        return None
    return ctx


def prepare_obfuscators(pub_key, count: int, chunk: int = DEFAULT_CHUNK) -> int:
    """Draw up to `count` obfuscators for pub_key now. Reserves the ring on first use and grows it only while it is
    empty; then fills in slices of `chunk` (an encryption that arrives during a fill waits for the slice in progress),
    each under a fresh 32-byte key from the OS. Returns the number of entries added: `count`, or the free room of a ring
    that still holds entries."""
    count, chunk = int(count), max(1, int(chunk))
    if count <= 0:
        return 0
    with lock:
        if not _gpu():
            q = _host.setdefault((pub_key.n, os.getpid()), collections.deque())
            n, nsq = pub_key.n, pub_key.nsquare
            q.extend(gmpy_math.powmod(secrets.randbelow(n - 1) + 1, n, nsq) for _ in range(count))
            return count
        from . import _native, _runtime
        ctx = _runtime.context(pub_key)
        cap, ready, _ = ctx.pool_info()
        if cap == 0 or (ready == 0 and count > cap):
            ctx.pool_reserve(count)
            cap = count
        _device[(pub_key.n, _runtime.device_index(), os.getpid())] = weakref.ref(ctx)
        todo = min(count, cap - ready)
    done = 0
    while done < todo:                                                # slice by slice: the lock is free in between
        with lock:
            cap, ready, _ = ctx.pool_info()
            n = min(chunk, todo - done, cap - ready)
            if n <= 0:
                break
            ctx.pool_fill(n, _native.PAI_OBF_RNG, rng_key=os.urandom(32), index_base=0)
        done += n
    return done


def obfuscators_ready(pub_key) -> int:
    """Ready obfuscators of pub_key in this process (0 when none were prepared)."""
    with lock:
        q = _host.get((pub_key.n, os.getpid()))
        if q is not None:
            return len(q)
        if not _device:
            return 0
        ctx = _device_ctx(pub_key)
        return ctx.pool_info()[1] if ctx is not None else 0


def device_pool(pub_key, count: int):
    """The native context to serve `count` elements with PAI_OBF_POOL, or None (no pool prepared, or fewer ready than the
    call needs). Callers hold `lock` from here until their call returns."""
    if not _device or count <= 0:
        return None
    ctx = _device_ctx(pub_key)
    if ctx is None or ctx.pool_info()[1] < count:
        return None
    return ctx


def host_pool_take(pub_key, count: int) -> List[int]:
    """Pop `count` obfuscators of the host pool, oldest first, or [] when it does not hold them all."""
    if not _host or count <= 0:
        return []
    with lock:
        q = _host.get((pub_key.n, os.getpid()))
        if q is None or len(q) < count:
            return []
        return [q.popleft() for _ in range(count)]


def drop(pub_key=None) -> None:
    """Forget the pools of pub_key (of every key: None). The device ring is freed."""
    with lock:
        for k in [k for k in _host if pub_key is None or k[0] == pub_key.n]:
            del _host[k]
        for k in [k for k in _device if pub_key is None or k[0] == pub_key.n]:
            ctx = _device.pop(k)()
            if ctx is not None:
                ctx.pool_reserve(0)
