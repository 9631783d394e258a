"""ctypes binding of libflexpai.so, the MI355X Paillier engine (C ABI: include/flexpai.h).

The shared library is built in-tree by ``__graft_entry__.build()`` (hipcc --offload-arch=gfx950)
and is REQUIRED: there is no CPU fallback. Loading fails loudly if it is missing.
"""
from __future__ import annotations

import collections
import ctypes
import os
import sys
import threading
import warnings
from typing import Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FLEXPAI_LIB") or os.path.join(_HERE, "libflexpai.so")   # override: experiments only
# the test-only build (FLEXPAI_XCHECK): also holds the kernel generations the tests still cross-check against
# (k_fbgp, k_pfb, k_fbp), selected by $FLEXPAI_SGP=0 / $FLEXPAI_FBS=0, and honours $FLEXPAI_PAIR=0
XCHECK_LIB_PATH = os.path.join(_HERE, "libflexpai_xcheck.so")

PAI_F32, PAI_F64, PAI_I64 = 0, 1, 2
PAI_OBF_NONE, PAI_OBF_GIVEN, PAI_OBF_RNG = 0, 1, 2
PAI_OBF_POOL = 3     # the call's obfuscators come from the context's pool (pai_pool_*), in order, each exactly once
PAI_EXP_AUTO, PAI_EXP_FIXED = 0, 1
EL_OK, EL_INT, EL_INT_BIG, EL_OVERFLOW, EL_FLOAT_OVF, EL_ENC_RANGE = 0, 1, 2, 3, 4, 5

PAI_OPT_CRT_ENCRYPT, PAI_OPT_CRT_AVAILABLE, PAI_OPT_STAGE_TIMING, PAI_OPT_LANE_DECRYPT = 1, 2, 3, 4
PAI_OPT_FIXED_BASE, PAI_OPT_FB_WINDOW, PAI_OPT_FB_READY, PAI_OPT_FB_PAIR, PAI_OPT_PAIR = 5, 6, 7, 8, 9
PAI_OPT_SPLIT_SAMPLER, PAI_OPT_ROWS_MAX = 13, 14
PAI_OPT_CRT4_MIN = 15
PAI_OPT_MATMUL_FUSED, PAI_OPT_MATMUL_PATH = 16, 17
PAI_OPT_OBF_CHUNK = 18
PAI_OPT_SEGDOT_FUSED, PAI_OPT_SEGDOT_PATH = 20, 21     # 19 is not assigned
PAI_OPT_POOL_FUSED = 22
PAI_BIN_U8, PAI_BIN_U16 = 0, 1
PAI_OPT_SCAN_TILE, PAI_OPT_SCAN_PATH = 23, 24
PAI_OPT_FOLD_ROWS, PAI_OPT_FOLD_PATH = 25, 26
PAI_SCAN_REVERSE = 1
HIST_RUN = 64          # PAI_HIST_RUN: members of a histogram cell that one k_hist_acc instance sums
PAI_OPT_PUBLIC_FB, PAI_OPT_PFB_READY, PAI_OPT_PFB_WINDOW = 10, 11, 12
PFB_NBASES = 33

EXPORTED = ("pai_device_count", "pai_device_mem_info", "pai_ctx_create", "pai_ctx_set_private", "pai_ctx_destroy", "pai_ctx_info", "pai_last_error",
            "pai_ctx_set_option", "pai_ctx_get_option", "pai_ctx_stage_times", "pai_ctx_fixed_base_info",
            "pai_ctx_fixed_base_prepare", "pai_ctx_fixed_base_setup", "pai_ctx_fixed_base_policy",
            "pai_ctx_public_fb_prepare", "pai_ctx_public_fb_set_bases", "pai_ctx_public_fb_info",
            "pai_ctx_public_fb_policy",
            "pai_encrypt", "pai_add", "pai_decrypt", "pai_encrypt_dev", "pai_add_dev", "pai_decrypt_dev",
            "pai_mul", "pai_mul_dev", "pai_matmul", "pai_matmul_dev", "pai_add_plain", "pai_add_plain_dev",
            "pai_segment_add", "pai_segment_add_dev", "pai_comm_unique_id", "pai_comm_create", "pai_comm_destroy",
            "pai_allgather_dev", "pai_allgather_shards_dev", "pai_release_table_cache", "pai_debug_encrypt_route",
            "pai_next_prime", "pai_prime_last_times", "pai_prime_test", "pai_debug_prime_sieve",
            "pai_obfuscate", "pai_obfuscate_dev",
            "pai_pack_max_slots", "pai_encrypt_packed", "pai_encrypt_packed_dev", "pai_decrypt_packed",
            "pai_decrypt_packed_dev", "pai_pack_ciphertexts", "pai_pack_ciphertexts_dev", "pai_repack", "pai_repack_dev",
            "pai_segment_dot", "pai_segment_dot_dev", "pai_histogram", "pai_histogram_dev",
            "pai_histogram_sparse", "pai_histogram_sparse_dev",
            "pai_cumsum", "pai_cumsum_dev",
            "pai_pool_reserve", "pai_pool_fill", "pai_pool_fill_dev", "pai_pool_put", "pai_pool_put_dev", "pai_pool_info",
            "pai_dev_alloc", "pai_dev_free", "pai_dev_upload", "pai_dev_download", "pai_dev_copy", "pai_dev_io_stats",
            "pai_dev_release_staging", "pai_take_dev", "pai_check_below_dev",
            "pai_take_idx_dev", "pai_segment_add_idx_dev")
RESIDENT = EXPORTED[-11:-2]   # device-resident buffers (include/flexpai.h)
DEVICE_INDEX = EXPORTED[-2:]  # take and segment sums over index lists that are device memory
PAI_COMM_ID_BYTES = 128

_lib = None
_libs = {}
_lib_lock = threading.Lock()


class NativeError(RuntimeError):
    pass


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libflexpai.so (or another build of the C ABI, e.g. XCHECK_LIB_PATH) and declare the C signatures.
    Raises if the library is absent."""
    global _lib
    with _lib_lock:
        if path in _libs:
            return _libs[path]
        if not os.path.exists(path):
            raise NativeError(f"flexpai native library not found at {path}; run __graft_entry__.build() "
                              f"(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        _start_torch_runtime_first()
        if "torch" not in sys.modules:
            _watch_late_torch_import()
        lib = ctypes.CDLL(path)
        P, S, I, U64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64
        lib.pai_device_count.argtypes = [P]
        lib.pai_device_mem_info.argtypes = [I, P, P]
        lib.pai_ctx_create.argtypes = [P, S, I, ctypes.POINTER(ctypes.c_void_p)]
        lib.pai_ctx_set_private.argtypes = [P, P, P, S]
        lib.pai_ctx_destroy.argtypes = [P]
        lib.pai_ctx_destroy.restype = None
        lib.pai_ctx_info.argtypes = [P, P, P, P]
        lib.pai_last_error.restype = ctypes.c_char_p
        lib.pai_ctx_set_option.argtypes = [P, I, I]
        lib.pai_ctx_get_option.argtypes = [P, I, P]
        lib.pai_ctx_stage_times.argtypes = [P, P, I, P]
        lib.pai_ctx_fixed_base_info.argtypes = [P, P, P, P, P]
        lib.pai_ctx_fixed_base_prepare.argtypes = [P]
        lib.pai_ctx_fixed_base_setup.argtypes = [P, P, P, P]
        lib.pai_ctx_fixed_base_policy.argtypes = [P, P, P]
        lib.pai_ctx_public_fb_prepare.argtypes = [P]
        lib.pai_ctx_public_fb_set_bases.argtypes = [P, P, S, I]
        lib.pai_ctx_public_fb_info.argtypes = [P, P, S, P, P, P, P]
        lib.pai_ctx_public_fb_policy.argtypes = [P, P, P]
        lib.pai_encrypt.argtypes = [P, I, P, S, I, ctypes.c_int32, I, P, S, S, P, U64, P, P, P]
        lib.pai_add.argtypes = [P, P, P, I, S, P, P]
        lib.pai_decrypt.argtypes = [P, P, P, S, P, P, P, P]
        lib.pai_encrypt_dev.argtypes = [P, I, P, S, I, ctypes.c_int32, I, P, S, S, P, U64, P, P, P, P]
        lib.pai_add_dev.argtypes = [P, P, P, I, S, P, P, P]
        lib.pai_decrypt_dev.argtypes = [P, P, P, S, P, P, P, P, P]
        lib.pai_obfuscate.argtypes = [P, P, S, I, P, S, S, P, U64, P]
        lib.pai_obfuscate_dev.argtypes = [P, P, S, I, P, S, S, P, U64, P, P]
        lib.pai_pool_reserve.argtypes = [P, S]
        lib.pai_pool_fill.argtypes = [P, S, I, P, S, S, P, U64]
        lib.pai_pool_fill_dev.argtypes = [P, S, I, P, S, S, P, U64, P]
        lib.pai_pool_put.argtypes = [P, P, S]
        lib.pai_pool_put_dev.argtypes = [P, P, S, P]
        lib.pai_pool_info.argtypes = [P, P, P, P]
        lib.pai_pack_max_slots.argtypes = [P, I, P]
        lib.pai_encrypt_packed.argtypes = [P, I, P, S, P, I, P, S, S, P, U64, P, P]
        lib.pai_encrypt_packed_dev.argtypes = [P, I, P, S, P, I, P, S, S, P, U64, P, P, P]
        lib.pai_decrypt_packed.argtypes = [P, P, P, S, P, P, P]
        lib.pai_decrypt_packed_dev.argtypes = [P, P, P, S, P, P, P, P]
        lib.pai_pack_ciphertexts.argtypes = [P, P, P, S, P, P, P]
        lib.pai_pack_ciphertexts_dev.argtypes = [P, P, P, S, P, P, P, P]
        lib.pai_repack.argtypes = [P, P, S, P, I, P]
        lib.pai_repack_dev.argtypes = [P, P, S, P, I, P, P]
        lib.pai_mul.argtypes = [P, P, P, S, I, P, S, P, P, P]
        lib.pai_mul_dev.argtypes = [P, P, P, S, I, P, S, P, P, P, P]
        lib.pai_add_plain.argtypes = [P, P, P, S, I, P, S, P, P, P]
        lib.pai_add_plain_dev.argtypes = [P, P, P, S, I, P, S, P, P, P, P]
        lib.pai_segment_add.argtypes = [P, P, P, S, P, P, S, P, P]
        lib.pai_segment_add_dev.argtypes = [P, P, P, S, P, P, S, P, P, P]
        lib.pai_segment_dot.argtypes = [P, P, P, S, P, P, S, I, P, P, P, P]
        lib.pai_segment_dot_dev.argtypes = [P, P, P, S, P, P, S, I, P, P, P, P, P]
        lib.pai_histogram.argtypes = [P, P, P, S, I, P, S, S, P, S, S, P, P, P]
        lib.pai_histogram_dev.argtypes = [P, P, P, S, I, P, S, S, P, S, S, P, P, P, P]
        lib.pai_histogram_sparse.argtypes = [P, P, P, S, P, P, I, P, S, P, P, S, S, P, P, P]
        lib.pai_histogram_sparse_dev.argtypes = [P, P, P, S, P, P, I, P, S, P, P, S, S, P, P, P, P]
        lib.pai_cumsum.argtypes = [P, P, P, S, S, S, I, P, P]
        lib.pai_cumsum_dev.argtypes = [P, P, P, S, S, S, I, P, P, P]
        lib.pai_matmul.argtypes = [P, P, P, S, S, I, P, S, P, P]
        lib.pai_matmul_dev.argtypes = [P, P, P, S, S, I, P, S, P, P, P]
        lib.pai_comm_unique_id.argtypes = [P]
        lib.pai_comm_create.argtypes = [P, I, I, I, ctypes.POINTER(ctypes.c_void_p)]
        lib.pai_comm_destroy.argtypes = [P]
        lib.pai_comm_destroy.restype = None
        lib.pai_allgather_dev.argtypes = [P, P, S, P, P]
        lib.pai_allgather_shards_dev.argtypes = [P, P, P, S, I, P, P, P]
        lib.pai_debug_encrypt_route.argtypes = [P, I, ctypes.c_longlong, I, P, P]
        lib.pai_release_table_cache.argtypes = []
        lib.pai_next_prime.argtypes = [I, I, P, S, S, ctypes.c_uint32, P, P]
        lib.pai_prime_last_times.argtypes = [P, P, P, P]
        lib.pai_prime_test.argtypes = [I, I, P, S, S, P, S, P]
        lib.pai_debug_prime_sieve.argtypes = [I, P, S, ctypes.c_uint32, P, S, P]
        lib.pai_release_table_cache.restype = None
        # (a library built from an earlier commit, loaded next to this one by the A/B tools, has no resident buffers)
        resident = hasattr(lib, "pai_dev_alloc")
        if resident:
            lib.pai_dev_alloc.argtypes = [I, S, ctypes.POINTER(ctypes.c_void_p)]
            lib.pai_dev_free.argtypes = [I, P]
            lib.pai_dev_upload.argtypes = [I, P, P, S]
            lib.pai_dev_download.argtypes = [I, P, P, S]
            lib.pai_dev_copy.argtypes = [I, P, P, S]
            lib.pai_dev_io_stats.argtypes = [P, P]
            lib.pai_dev_release_staging.argtypes = []
            lib.pai_take_dev.argtypes = [P, P, P, S, P, S, P, P, P]
            lib.pai_check_below_dev.argtypes = [P, P, S, P, P]
        device_index = hasattr(lib, "pai_take_idx_dev")
        if device_index:
            lib.pai_take_idx_dev.argtypes = [P, P, P, S, P, S, I, P, P, P, P]
            lib.pai_segment_add_idx_dev.argtypes = [P, P, P, S, P, S, P, S, P, P, P, P]
        for name in EXPORTED:
            if (not resident and name in RESIDENT) or (not device_index and name in DEVICE_INDEX):
                continue
            if name not in ("pai_ctx_destroy", "pai_last_error", "pai_comm_destroy", "pai_release_table_cache"):
                getattr(lib, name).restype = ctypes.c_int
        _libs[path] = lib
        if path == LIB_PATH:
            _lib = lib
        return lib


def release_staging() -> None:
    """Give the pinned staging slots, copy streams and events of the device-buffer transfers back now
    (pai_dev_release_staging: up to 128 MiB of pinned host memory per device; the next transfer makes them again)."""
    lib = load_library()
    _check(lib.pai_dev_release_staging(), lib)


def release_table_cache() -> None:
    """Give the device memory of released fixed-base tables back to the driver now (csrc/table_arena.hpp: the library
    keeps it for the process's next table build until its last context is destroyed)."""
    load_library().pai_release_table_cache()


def _start_torch_runtime_first() -> None:
    """PyTorch-ROCm wheels bundle their own HIP and HSA runtimes. In one process only the runtime that opens the
    GPU first works: once libflexpai's (/opt/rocm) runtime has started, torch.cuda fails with "No HIP GPUs are
    available". A process that has already imported torch (device buffers for the *_dev entry points, a
    torch.distributed job) gets torch's runtime started here, before flexpai's first HIP call; torch is never
    imported by this package. See INTEGRATION.md (PyTorch)."""
    import sys
    torch = sys.modules.get("torch")
    if torch is None or os.environ.get("FLEXPAI_NO_TORCH_INIT"):
        return
    try:
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:   # noqa: BLE001 - torch without a usable GPU: flexpai's own runtime still works
        pass


_runtime_started = False   # a context was created: libflexpai's HIP runtime holds the GPU
_torch_watch = None


class _LateTorchWatch:
    """sys.meta_path finder armed when libflexpai loads before torch: when torch is imported later, after
    libflexpai's runtime has opened the GPU, torch's own HIP runtime cannot (torch.cuda.is_available() is False).
    Warn once at that import instead of leaving the caller to find the failure. One shot:
    the finder removes itself at torch's import and never changes what is imported."""

    def find_spec(self, name, path=None, target=None):
        if name != "torch":
            return None
        _disarm_torch_watch()
        import importlib.machinery
        spec = importlib.machinery.PathFinder.find_spec(name, path)
        loader = getattr(spec, "loader", None)
        if loader is None or not hasattr(loader, "exec_module"):
            return spec
        inner = loader.exec_module

        def exec_module(module):
            inner(module)
            _check_torch_after_flexpai(module)

        loader.exec_module = exec_module   # (this loader instance only: it loads torch's __init__ and nothing else)
        return spec


def _watch_late_torch_import() -> None:
    global _torch_watch
    if _torch_watch is None and not os.environ.get("FLEXPAI_NO_TORCH_INIT"):
        _torch_watch = _LateTorchWatch()
        sys.meta_path.insert(0, _torch_watch)


def _disarm_torch_watch() -> None:
    global _torch_watch
    if _torch_watch is not None:
        try:
            sys.meta_path.remove(_torch_watch)
        except ValueError:
            pass
        _torch_watch = None


def _check_torch_after_flexpai(torch) -> bool:
    """True (and a RuntimeWarning) when torch was imported after libflexpai started the GPU and torch cannot see it."""
    if not _runtime_started:
        return False
    try:
        ok = bool(torch.cuda.is_available())
    except Exception:   # noqa: BLE001 - a torch without a HIP build: nothing of ours to report
        return False
    if ok:
        return False
    warnings.warn("flexpai: torch was imported after libflexpai started the GPU, and torch.cuda now reports no GPU "
                  "(two HIP runtimes in one process: the first to open the device keeps it). Import torch before "
                  "the first Paillier call; see INTEGRATION.md (PyTorch).", RuntimeWarning, stacklevel=2)
    return True


def device_count() -> int:
    """GPUs visible to the engine (0 without one). Raises when libflexpai.so is missing."""
    n = ctypes.c_int()
    _check(load_library().pai_device_count(ctypes.byref(n)))
    return n.value


def device_mem_info(device: int = 0):
    """(free, total) device memory in bytes, through the engine's own HIP runtime."""
    fr, tot = ctypes.c_uint64(), ctypes.c_uint64()
    _check(load_library().pai_device_mem_info(device, ctypes.byref(fr), ctypes.byref(tot)))
    return fr.value, tot.value


class DeviceMem:
    """A block of device memory of the library (pai_dev_alloc; include/flexpai.h, "Device-resident ciphertext
    buffers"): owned by the device, not by a context. free() -- and the finaliser -- wait for the device's queued work
    before the block goes back. DeviceMem.wrap(ptr, nbytes, device, owner) names memory somebody else owns (a torch
    tensor's data_ptr()): it keeps `owner` alive and never frees."""
    __slots__ = ("ptr", "nbytes", "device", "owner", "_lib")

    def __init__(self, nbytes: int, device: int = 0, lib=None):
        self._lib = lib or load_library()
        self.nbytes, self.device, self.owner = int(nbytes), int(device), None
        p = ctypes.c_void_p()
        _check(self._lib.pai_dev_alloc(self.device, self.nbytes, ctypes.byref(p)), self._lib)
        global _runtime_started
        _runtime_started = True
        self.ptr = p.value or 0

    @classmethod
    def wrap(cls, ptr: int, nbytes: int, device: int = 0, owner=None) -> "DeviceMem":
        m = object.__new__(cls)
        m._lib, m.ptr, m.nbytes, m.device, m.owner = None, int(ptr), int(nbytes), int(device), owner
        return m

    def at(self, offset: int) -> int:
        return self.ptr + int(offset)

    def upload(self, a: np.ndarray, offset: int = 0) -> "DeviceMem":
        """Host array -> this block at byte `offset` (pai_dev_upload: pinned staging, complete on return)."""
        a = np.ascontiguousarray(a)
        if offset < 0 or offset + a.nbytes > self.nbytes:
            raise ValueError("upload: the array does not fit the device block")
        lib = self._lib or load_library()
        if a.nbytes:
            _check(lib.pai_dev_upload(self.device, self.ptr + offset, _ptr(a), a.nbytes), lib)
        return self

    def download(self, dtype, count: int, offset: int = 0) -> np.ndarray:
        """`count` elements of `dtype` from byte `offset` (pai_dev_download; waits for the device's queued work)."""
        out = np.empty(int(count), dtype=dtype)
        if offset < 0 or offset + out.nbytes > self.nbytes:
            raise ValueError("download: the range lies outside the device block")
        lib = self._lib or load_library()
        if out.nbytes:
            _check(lib.pai_dev_download(self.device, _ptr(out), self.ptr + offset, out.nbytes), lib)
        return out

    def copy_from(self, src: "DeviceMem", nbytes: int, offset: int = 0, src_offset: int = 0) -> "DeviceMem":
        """Device-to-device copy (pai_dev_copy) of `nbytes` from src at src_offset to this block at offset."""
        if min(offset, src_offset, nbytes) < 0 or offset + nbytes > self.nbytes or src_offset + nbytes > src.nbytes:
            raise ValueError("copy_from: the range lies outside a device block")
        if src.device != self.device:
            raise ValueError("copy_from: the blocks are on different devices")
        lib = self._lib or load_library()
        if nbytes:
            _check(lib.pai_dev_copy(self.device, self.ptr + offset, src.ptr + src_offset, int(nbytes)), lib)
        return self

    def free(self) -> None:
        if self._lib is not None and self.ptr:
            lib, p = self._lib, self.ptr
            self.ptr = 0
            _check(lib.pai_dev_free(self.device, p), lib)
        self.ptr, self.owner = 0, None

    def __del__(self):
        try:
            self.free()
        except Exception:   # noqa: BLE001 - interpreter shutdown
            pass


def device_upload(a: np.ndarray, device: int = 0) -> DeviceMem:
    """A fresh device block holding the host array `a`."""
    a = np.ascontiguousarray(a)
    return DeviceMem(a.nbytes, device).upload(a)


def dev_io_stats(lib=None) -> Tuple[int, int]:
    """(host-to-device, device-to-host) bytes moved by pai_dev_upload / pai_dev_download in this process (per loaded
    build of the library)."""
    lib = lib or load_library()
    up, down = ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib.pai_dev_io_stats(ctypes.byref(up), ctypes.byref(down)), lib)
    return int(up.value), int(down.value)


class Comm:
    """RCCL communicator of the C ABI's shard all-gather (pai_comm_*): one per rank, one process per GPU.
    Rank 0 makes the id (Comm.unique_id()) and passes it to the others over any channel."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (ctypes.c_uint8 * PAI_COMM_ID_BYTES)()
        _check(load_library().pai_comm_unique_id(buf))
        return bytes(buf)

    def _chk(self, rc: int):
        _check(rc, self.lib)

    def __init__(self, uid: bytes, world: int, rank: int, device: int = 0):
        if len(uid) != PAI_COMM_ID_BYTES:
            raise ValueError("communicator id must be %d bytes" % PAI_COMM_ID_BYTES)
        self.lib = load_library()
        h = ctypes.c_void_p()
        self._chk(self.lib.pai_comm_create(uid, world, rank, device, ctypes.byref(h)))
        self._h, self.world, self.rank = h, world, rank

    def allgather_shards(self, d_ct: int, d_exp: int, n_per_rank: int, ct_words: int, d_ct_all: int,
                         d_exp_all: int, stream: int = 0):
        """Device pointers (e.g. torch tensor .data_ptr()); asynchronous on `stream`."""
        self._chk(self.lib.pai_allgather_shards_dev(self._h, d_ct, d_exp, n_per_rank, ct_words, d_ct_all, d_exp_all,
                                                 stream or None))

    def close(self):
        if getattr(self, "_h", None):
            self.lib.pai_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check(rc: int, lib=None):
    if rc != 0:
        msg = (lib or load_library()).pai_last_error().decode(errors="replace")
        if rc == -5:
            raise ZeroDivisionError(msg)          # gmpy_math.invert (gmpy_math.py:71-72)
        if rc == -4 and ("does not match" in msg or "have to be different" in msg):
            raise ValueError(msg)
        raise NativeError(f"flexpai error {rc}: {msg}")


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def int_to_le(v: int, nbytes: int) -> bytes:
    return int(v).to_bytes(nbytes, "little")


class Context:
    """One key on one GPU. Created lazily by the Python layer (never pickled, never forked)."""

    def __init__(self, n: int, device: int = 0, p: Optional[int] = None, q: Optional[int] = None, lib=None):
        """lib: another build of the C ABI (load_library(XCHECK_LIB_PATH) in the cross-check tests)."""
        self.lib = lib or load_library()
        self.n = n
        self.device = int(device)
        nbytes = (n.bit_length() + 7) // 8
        buf = int_to_le(n, nbytes)
        h = ctypes.c_void_p()
        self._chk(self.lib.pai_ctx_create(buf, nbytes, device, ctypes.byref(h)))
        global _runtime_started
        _runtime_started = True
        self._h = h
        kb, cw, pw = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._chk(self.lib.pai_ctx_info(h, ctypes.byref(kb), ctypes.byref(cw), ctypes.byref(pw)))
        self.key_bits, self.ct_words, self.pt_words = kb.value, cw.value, pw.value
        self.has_private = False
        self.calls = collections.Counter()     # C-ABI entry points this context has run (tests, stats)
        if p is not None:
            self.set_private(p, q)

    def _chk(self, rc: int):
        _check(rc, self.lib)

    @property
    def handle(self):
        return self._h

    def set_private(self, p: int, q: int):
        hb = max(p.bit_length(), q.bit_length()) // 8 + 1
        self._chk(self.lib.pai_ctx_set_private(self._h, int_to_le(p, hb), int_to_le(q, hb), hb))
        self.has_private = True
        if os.environ.get("FLEXPAI_CRT", "1").strip() == "0":
            self.set_crt(False)

    def _get_option(self, opt: int) -> int:
        v = ctypes.c_int()
        self._chk(self.lib.pai_ctx_get_option(self._h, opt, ctypes.byref(v)))
        return v.value

    @property
    def crt_available(self) -> bool:
        """True when the private key is set and the CRT encryption kernels fit this key size."""
        return bool(self._get_option(PAI_OPT_CRT_AVAILABLE))

    @property
    def crt_enabled(self) -> bool:
        return bool(self._get_option(PAI_OPT_CRT_ENCRYPT))

    def set_stage_timing(self, enabled: bool):
        self._chk(self.lib.pai_ctx_set_option(self._h, PAI_OPT_STAGE_TIMING, 1 if enabled else 0))

    def stage_times(self):
        """Kernel durations (ms) of the last encrypt call (needs set_stage_timing(True))."""
        buf = (ctypes.c_float * 8)()
        cnt = ctypes.c_int()
        self._chk(self.lib.pai_ctx_stage_times(self._h, buf, 8, ctypes.byref(cnt)))
        return [float(buf[i]) for i in range(cnt.value)]

    @property
    def rows_max(self) -> int:
        """Largest CRT encryption / decryption call (elements) that runs on 16-lane rows (k_crt_w / k_dec_w)."""
        return int(self._get_option(PAI_OPT_ROWS_MAX))

    def set_rows_max(self, n: int):
        """0 keeps every CRT encryption / decryption on the lane kernels (k_crt_a + k_crt_b_pair, k_dec_*_pair); same bits."""
        self._chk(self.lib.pai_ctx_set_option(self._h, PAI_OPT_ROWS_MAX, int(n)))

    @property
    def crt4_min(self) -> int:
        """A 2049..4096-bit key holder's calls of at most this many elements (default 128) that the rows do not take stay
        on k_encrypt<8> instead of the split-pair CRT (kernels_crt4.hpp)."""
        return int(self._get_option(PAI_OPT_CRT4_MIN))

    def set_crt4_min(self, n: int):
        """0 sends every call above the rows through the split-pair CRT; same bits."""
        self._chk(self.lib.pai_ctx_set_option(self._h, PAI_OPT_CRT4_MIN, int(n)))

    @property
    def matmul_fused(self) -> bool:
        """True when matmul runs the fused windowed multi-exponentiation (kernels_mm.hpp: the default, for products of
        d >= 16 columns that fill the chip), False for one k_mul exponentiation per term on every call."""
        return bool(self._get_option(PAI_OPT_MATMUL_FUSED))

    def set_matmul_fused(self, enabled: bool):
        """False keeps matmul on k_mul + batch inversion + k_add over all K m d terms; same bits."""
        self._chk(self.lib.pai_ctx_set_option(self._h, PAI_OPT_MATMUL_FUSED, 1 if enabled else 0))

    @property
    def matmul_path(self) -> int:
        """The path of this context's last matmul call: 0 = none yet, 1 = term path, 2 = fused."""
        return int(self._get_option(PAI_OPT_MATMUL_PATH))

    @property
    def segdot_fused(self) -> bool:
        """True when segment_dot may run the fused windowed multi-exponentiation (kernels_sd.hpp: the default, for calls
        with enough reuse per distinct ciphertext and enough chunks to fill the chip), False for the term path always."""
        return bool(self._get_option(PAI_OPT_SEGDOT_FUSED))

    def set_segdot_fused(self, enabled: bool):
        """False keeps segment_dot on gather + k_mul + batch inversion + segmented add over all entries; same bits."""
        self._chk(self.lib.pai_ctx_set_option(self._h, PAI_OPT_SEGDOT_FUSED, 1 if enabled else 0))

    @property
    def segdot_path(self) -> int:
        """The path of this context's last segment_dot call: 0 = none yet, 1 = term path, 2 = fused."""
        return int(self._get_option(PAI_OPT_SEGDOT_PATH))

    @property
    def scan_tile(self) -> int:
        """Tile length of cumsum's blocked path; 0 = automatic."""
        return int(self._get_option(PAI_OPT_SCAN_TILE))

    def set_scan_tile(self, n: int):
        """0: automatic; n > 0: tiles of n elements at every level of the scan. Same bits for every value."""
        self._chk(self.lib.pai_ctx_set_option(self._h, PAI_OPT_SCAN_TILE, int(n)))

    @property
    def scan_path(self) -> int:
        """The path of this context's last cumsum call: 0 = none yet, 1 = row chains, 2 = blocked scan."""
        return int(self._get_option(PAI_OPT_SCAN_PATH))

    @property
    def fold_rows(self) -> int:
        """pack_ciphertexts / repack on 16-lane rows: 1 = automatic (calls of few outputs), 0 = never, 2 = always."""
        return int(self._get_option(PAI_OPT_FOLD_ROWS))

    def set_fold_rows(self, mode: int):
        """0: lane groups only; 1: automatic; 2: rows wherever a row kernel exists. Same bits for every value."""
        self._chk(self.lib.pai_ctx_set_option(self._h, PAI_OPT_FOLD_ROWS, int(mode)))

    @property
    def fold_path(self) -> int:
        """The path of this context's last pack_ciphertexts or repack call: 0 = none yet, 1 = lane groups, 2 = rows."""
        return int(self._get_option(PAI_OPT_FOLD_PATH))

    @property
    def obf_chunk(self) -> int:
        """Elements per slice of an in-place pai_obfuscate_dev (default 262 144)."""
        return int(self._get_option(PAI_OPT_OBF_CHUNK))

    def set_obf_chunk(self, n: int):
        """At least 64; same bits for every value."""
        self._chk(self.lib.pai_ctx_set_option(self._h, PAI_OPT_OBF_CHUNK, int(n)))

    def set_crt(self, enabled: bool):
        """Encrypt through the private-key CRT kernels (default when available) or the public-key one.
        The ciphertext bits are identical either way."""
        self._chk(self.lib.pai_ctx_set_option(self._h, PAI_OPT_CRT_ENCRYPT, 1 if enabled else 0))

    @property
    def lane_decrypt(self) -> bool:
        """True when decrypt runs on the lane engine (kernels_dec.hpp), False for the lane-group kernel."""
        return bool(self._get_option(PAI_OPT_LANE_DECRYPT))

    def set_lane_decrypt(self, enabled: bool):
        self._chk(self.lib.pai_ctx_set_option(self._h, PAI_OPT_LANE_DECRYPT, 1 if enabled else 0))

    @property
    def fixed_base(self) -> bool:
        """True when device-RNG encryption samples r^n through the fixed bases (kernels_fb.hpp)."""
        return bool(self._get_option(PAI_OPT_FIXED_BASE))

    def set_fixed_base(self, enabled: bool):
        self._chk(self.lib.pai_ctx_set_option(self._h, PAI_OPT_FIXED_BASE, 1 if enabled else 0))

    def fixed_base_info(self):
        """(g_p, g_q, K, W): the generators, the exponent digit count and the digit window (bits) of
        the fixed-base path."""
        gp, gq, k, w = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_int(), ctypes.c_int()
        self._chk(self.lib.pai_ctx_fixed_base_info(self._h, ctypes.byref(gp), ctypes.byref(gq), ctypes.byref(k),
                                                ctypes.byref(w)))
        return gp.value, gq.value, k.value, w.value

    @property
    def fb_window(self) -> int:
        """Window of the resident fixed-base tables (else the requested one)."""
        return self._get_option(PAI_OPT_FB_WINDOW)

    def set_fb_window(self, bits: int):
        """Digit window of the fixed-base tables (8, 12, 16 or 20 .. 24); the tables are rebuilt lazily."""
        self._chk(self.lib.pai_ctx_set_option(self._h, PAI_OPT_FB_WINDOW, int(bits)))

    @property
    def fb_ready(self) -> bool:
        """True when the fixed-base tables are resident on the device."""
        return bool(self._get_option(PAI_OPT_FB_READY))

    @property
    def fb_pair(self) -> int:
        """Limbs of p_h of the resident pair tables (kernels_fbs.hpp: k_fbs; kernels_fbp.hpp: k_fbp in the test build),
        0 for k_fb tables or none."""
        return int(self._get_option(PAI_OPT_FB_PAIR))

    @property
    def split_sampler(self) -> int:
        """Bit 0: the 4096-bit key-holder tables, bit 1: the public tables are sampled by k_sgp (kernels_sgp.hpp);
        bit 2: the 1024/2048-bit key-holder tables hold Shoup rows sampled by k_fbs (kernels_fbs.hpp)."""
        return int(self._get_option(PAI_OPT_SPLIT_SAMPLER))

    @property
    def pair_paths(self) -> int:
        """Bit 0: decryption, bit 1: CRT encryption stage B on p-adic pairs (kernels_pair.hpp); bit 2: public-key
        encryption on pairs (n of at most 1024 bits and of 1537..2048 bits -- of the latter only keys of 128 ciphertext
        words, 2033..2048 bits, run k_pe_*, the others k_encrypt; n of 2049..4096 bits on pair groups,
        kernels_pe4.hpp, while the context holds no private key); bit 3: a 2049..4096-bit key holder's encryption above the
        rows runs the split-pair CRT (kernels_crt4.hpp)."""
        return int(self._get_option(PAI_OPT_PAIR))

    def prepare_fixed_base(self):
        """Build the fixed-base tables now (NativeError with the reason when unavailable)."""
        self._chk(self.lib.pai_ctx_fixed_base_prepare(self._h))

    def fixed_base_setup(self):
        """(host_ms, device_ms, table_bytes) of the last table build."""
        hm, dm, tb = ctypes.c_float(), ctypes.c_float(), ctypes.c_uint64()
        self._chk(self.lib.pai_ctx_fixed_base_setup(self._h, ctypes.byref(hm), ctypes.byref(dm), ctypes.byref(tb)))
        return float(hm.value), float(dm.value), int(tb.value)

    def fixed_base_policy(self):
        """(seen, threshold): device-RNG elements encrypted under this key so far, and the count at which
        the fixed-base tables get built (0 once resident or unavailable); include/flexpai.h."""
        seen, thr = ctypes.c_longlong(), ctypes.c_longlong()
        self._chk(self.lib.pai_ctx_fixed_base_policy(self._h, ctypes.byref(seen), ctypes.byref(thr)))
        return int(seen.value), int(thr.value)

    # ------------------------------------------------------ public-key fixed bases (kernels_pfb.hpp)
    @property
    def public_fixed_base(self) -> bool:
        """True when device-RNG encryption without the private key may use the public fixed bases."""
        return bool(self._get_option(PAI_OPT_PUBLIC_FB))

    def set_public_fixed_base(self, enabled: bool):
        self._chk(self.lib.pai_ctx_set_option(self._h, PAI_OPT_PUBLIC_FB, 1 if enabled else 0))

    @property
    def pfb_ready(self) -> bool:
        return bool(self._get_option(PAI_OPT_PFB_READY))

    def set_pfb_window(self, bits: int):
        """Digit window of the public tables: 12, 16 or 20 (the windows pinned to the reference's goldens)."""
        self._chk(self.lib.pai_ctx_set_option(self._h, PAI_OPT_PFB_WINDOW, int(bits)))

    def prepare_public_fixed_base(self):
        self._chk(self.lib.pai_ctx_public_fb_prepare(self._h))

    def set_public_bases(self, bases: Sequence[int]):
        """Fix the 33 bases g_0..g_32 instead of drawing them (tests, reproducible runs). Each must be a unit
        in (1, n), all distinct, and g_0 must have Jacobi symbol -1 mod n (else NativeError)."""
        nb = (self.n.bit_length() + 7) // 8
        buf = b"".join(int_to_le(g, nb) for g in bases)
        self._chk(self.lib.pai_ctx_public_fb_set_bases(self._h, buf, nb, len(bases)))

    def public_fixed_base_info(self):
        """(bases, K, W, K0) of the resident public tables."""
        nb = (self.n.bit_length() + 7) // 8
        buf = (ctypes.c_uint8 * (nb * PFB_NBASES))()
        nbs, k, w, k0 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._chk(self.lib.pai_ctx_public_fb_info(self._h, buf, nb, ctypes.byref(nbs), ctypes.byref(k), ctypes.byref(w),
                                               ctypes.byref(k0)))
        raw = bytes(buf)
        bases = [int.from_bytes(raw[j * nb:(j + 1) * nb], "little") for j in range(nbs.value)]
        return bases, k.value, w.value, k0.value

    def public_fixed_base_policy(self):
        seen, thr = ctypes.c_longlong(), ctypes.c_longlong()
        self._chk(self.lib.pai_ctx_public_fb_policy(self._h, ctypes.byref(seen), ctypes.byref(thr)))
        return int(seen.value), int(thr.value)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.pai_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check_words(self, ct: np.ndarray, exp: np.ndarray, N: int):
        """Host buffers must be exactly [N, ct_words] words and N exponents: the C ABI reads N * ct_words."""
        if ct.dtype != np.uint32 or ct.shape != (N, self.ct_words) or exp.shape != (N,):
            raise ValueError(f"ciphertext buffer shape {ct.shape} / exponents {exp.shape} do not match "
                             f"({N}, {self.ct_words})")

    # ----------------------------------------------------------------- device-pointer ops (device_buffer.py)
    def dev_call(self, name: str, *args) -> None:
        """The *_dev entry point `name` on device pointers (ints, DeviceMem.at()), on the null stream; asynchronous as
        include/flexpai.h states for that entry point. The callers (device_buffer.py) own the shapes."""
        self.calls[name] += 1
        self._chk(getattr(self.lib, name)(self._h, *args, None))

    def take_dev(self, d_ct: int, d_exp: int, N: int, index: np.ndarray, d_ct_out: int, d_exp_out: int) -> None:
        """pai_take_dev: out[j] = in[index[j]] (host int64 index; -1: ciphertext 1, exponent INT32_MIN)."""
        index = np.ascontiguousarray(index, dtype=np.int64).reshape(-1)
        self.dev_call("pai_take_dev", d_ct, d_exp, int(N), _ptr(index), index.size, d_ct_out, d_exp_out)

    def take_idx_dev(self, d_ct: int, d_exp: int, N: int, d_index: int, M: int, allow_empty: bool, d_ct_out: int,
                     d_exp_out: int, d_bad: int) -> None:
        """pai_take_idx_dev: out[j] = in[index[j]] for an int64 index in device memory; d_bad names two device int64 words
        (the smallest bad position or -1; -1). Nothing is waited for."""
        self.dev_call("pai_take_idx_dev", d_ct, d_exp, int(N), d_index, int(M), 1 if allow_empty else 0, d_ct_out,
                      d_exp_out, d_bad)

    def segment_add_idx_dev(self, d_ct: int, d_exp: int, N: int, d_index: int, total: int, d_seg_off: int, nseg: int,
                            d_out: int, d_exp_out: int, d_bad: int) -> None:
        """pai_segment_add_idx_dev: per-segment sums over an int64 index and nseg + 1 int64 offsets in device memory;
        d_bad names two device int64 words (the smallest bad index position, the smallest bad offset position, or -1)."""
        self.dev_call("pai_segment_add_idx_dev", d_ct, d_exp, int(N), d_index, int(total), d_seg_off, int(nseg), d_out,
                      d_exp_out, d_bad)

    def check_below_dev(self, d_ct: int, N: int) -> int:
        """pai_check_below_dev: the smallest i with ct[i] >= n^2, or -1."""
        first = ctypes.c_int64(-1)
        self.dev_call("pai_check_below_dev", d_ct, int(N), ctypes.byref(first))
        return int(first.value)

    # ----------------------------------------------------------------- host-buffer ops
    def encrypt(self, x: np.ndarray, exp_mode: int = PAI_EXP_AUTO, fixed_exp: int = 0,
                obf_mode: int = PAI_OBF_RNG, r: Optional[Sequence[int]] = None, r_scalar: Optional[int] = None,
                rng_key: Optional[bytes] = None, index_base: int = 0,
                out: Optional[Tuple[np.ndarray, np.ndarray, np.ndarray]] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Host buffers in and out. `out` = (ct [N, W] uint32, exp [N] int32, status [N] int32) to reuse
        caller buffers (a streaming sender's), else fresh arrays."""
        x = np.ascontiguousarray(x)
        if x.dtype == np.float32:
            dt = PAI_F32
        elif x.dtype == np.float64:
            dt = PAI_F64
        elif x.dtype == np.int64:
            dt = PAI_I64
        else:
            raise TypeError(f"unsupported dtype {x.dtype}")
        N = x.size
        if out is not None:
            ct, ex, st = out
            if not (ct.dtype == np.uint32 and ct.shape == (N, self.ct_words) and ct.flags.c_contiguous and
                    ex.dtype == np.int32 and ex.shape == (N,) and ex.flags.c_contiguous and
                    st.dtype == np.int32 and st.shape == (N,) and st.flags.c_contiguous):
                raise ValueError("out must be C-contiguous (uint32 [N, ct_words], int32 [N], int32 [N])")
        else:
            ct = np.empty((N, self.ct_words), dtype=np.uint32)
            ex = np.empty(N, dtype=np.int32)
            st = np.empty(N, dtype=np.int32)
        r_buf, r_stride, r_bytes = None, 0, 0
        if obf_mode == PAI_OBF_GIVEN:
            r_bytes = self.ct_words * 4
            if r_scalar is not None:
                r_buf = np.frombuffer(int_to_le(r_scalar, r_bytes), dtype=np.uint8).copy()
                r_stride = 0
            else:
                r_buf = np.frombuffer(b"".join(int_to_le(v, r_bytes) for v in r), dtype=np.uint8).copy()
                r_stride = r_bytes
        key = rng_key if rng_key is not None else os.urandom(32)
        self.calls["pai_encrypt"] += 1
        self._chk(self.lib.pai_encrypt(self._h, dt, _ptr(x), N, exp_mode, fixed_exp, obf_mode,
                                    _ptr(r_buf) if r_buf is not None else None, r_stride, r_bytes,
                                    key, index_base, _ptr(ct), _ptr(ex), _ptr(st)))
        return ct, ex, st

    def obfuscate(self, ct: np.ndarray, obf_mode: int = PAI_OBF_RNG, r: Optional[Sequence[int]] = None,
                  r_scalar: Optional[int] = None, rng_key: Optional[bytes] = None, index_base: int = 0,
                  out: Optional[np.ndarray] = None) -> np.ndarray:
        """ct_i * r_i^n mod n^2 over [N, ct_words] words (pai_obfuscate; include/flexpai.h states which r). `out` may
        be `ct` itself (in place) or another C-contiguous uint32 [N, ct_words] array, else a fresh one. Returns the
        words."""
        ct = np.ascontiguousarray(ct, dtype=np.uint32)
        if ct.ndim != 2 or ct.shape[1] != self.ct_words:
            raise ValueError(f"ciphertext buffer shape {ct.shape} does not match (N, {self.ct_words})")
        N = ct.shape[0]
        if out is None:
            out = np.empty_like(ct)
        elif not (out.dtype == np.uint32 and out.shape == ct.shape and out.flags.c_contiguous):
            raise ValueError("out must be C-contiguous uint32 [N, ct_words]")
        r_buf, r_stride, r_bytes = None, 0, 0
        if obf_mode == PAI_OBF_GIVEN:
            r_bytes = self.ct_words * 4
            if r_scalar is not None:
                r_buf = np.frombuffer(int_to_le(r_scalar, r_bytes), dtype=np.uint8).copy()
            else:
                r_buf = np.frombuffer(b"".join(int_to_le(v, r_bytes) for v in r), dtype=np.uint8).copy()
                r_stride = r_bytes
        key = rng_key if rng_key is not None else os.urandom(32)
        self.calls["pai_obfuscate"] += 1
        self._chk(self.lib.pai_obfuscate(self._h, _ptr(ct), N, obf_mode, _ptr(r_buf) if r_buf is not None else None,
                                         r_stride, r_bytes, key, index_base, _ptr(out)))
        return out

    # ----------------------------------------------------------------- obfuscator pool (include/flexpai.h)
    def pool_reserve(self, capacity: int):
        """(Re)allocate the ring of ready obfuscators for `capacity` entries, dropping its contents; 0 frees it."""
        self._chk(self.lib.pai_pool_reserve(self._h, int(capacity)))

    def pool_fill(self, count: int, obf_mode: int = PAI_OBF_RNG, r: Optional[Sequence[int]] = None,
                  r_scalar: Optional[int] = None, rng_key: Optional[bytes] = None, index_base: int = 0):
        """Append `count` entries: entry j is what encrypt writes for the integer 0 at global index index_base + j with
        this obf_mode (PAI_OBF_GIVEN or PAI_OBF_RNG) and r or key, by that encryption's route."""
        r_buf, r_stride, r_bytes = None, 0, 0
        if obf_mode == PAI_OBF_GIVEN:
            r_bytes = self.ct_words * 4
            if r_scalar is not None:
                r_buf = np.frombuffer(int_to_le(r_scalar, r_bytes), dtype=np.uint8).copy()
            else:
                r_buf = np.frombuffer(b"".join(int_to_le(v, r_bytes) for v in r), dtype=np.uint8).copy()
                r_stride = r_bytes
        key = rng_key if rng_key is not None else os.urandom(32)
        self.calls["pai_pool_fill"] += 1
        self._chk(self.lib.pai_pool_fill(self._h, int(count), obf_mode, _ptr(r_buf) if r_buf is not None else None,
                                         r_stride, r_bytes, key, index_base))

    def pool_put(self, rho):
        """Append caller-made obfuscators: [count, ct_words] uint32 words, or a sequence of ints, each < n^2."""
        if not isinstance(rho, np.ndarray):
            rho = ints_to_words(rho, self.ct_words)
        rho = np.ascontiguousarray(rho, dtype=np.uint32)
        if rho.ndim != 2 or rho.shape[1] != self.ct_words:
            raise ValueError(f"obfuscator buffer shape {rho.shape} does not match (count, {self.ct_words})")
        self.calls["pai_pool_put"] += 1
        self._chk(self.lib.pai_pool_put(self._h, _ptr(rho), rho.shape[0]))

    def pool_info(self) -> Tuple[int, int, int]:
        """(capacity, ready, taken_total)."""
        cap, ready, taken = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self.lib.pai_pool_info(self._h, ctypes.byref(cap), ctypes.byref(ready), ctypes.byref(taken)))
        return int(cap.value), int(ready.value), int(taken.value)

    @property
    def pool_fused(self) -> bool:
        """True when pooled encryption runs k_pool_enc (the default), False for k_pool_join + the PAI_OBF_NONE
        encryption + k_obf_mul."""
        return bool(self._get_option(PAI_OPT_POOL_FUSED))

    def set_pool_fused(self, enabled: bool):
        """Same bits either way."""
        self._chk(self.lib.pai_ctx_set_option(self._h, PAI_OPT_POOL_FUSED, 1 if enabled else 0))

    # ----------------------------------------------------------------- packed plaintexts (include/flexpai.h)
    def pack_max_slots(self, slot_bits: int) -> int:
        """floor((key_bits - 2) / slot_bits), the most slots a layout of this key may have."""
        k = ctypes.c_int()
        self._chk(self.lib.pai_pack_max_slots(self._h, int(slot_bits), ctypes.byref(k)))
        return k.value

    def encrypt_packed(self, x: np.ndarray, layout, obf_mode: int = PAI_OBF_RNG, r: Optional[Sequence[int]] = None,
                       rng_key: Optional[bytes] = None, index_base: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """pai_encrypt_packed: x (float32 / float64 / int64) into ceil(N / slots) ciphertexts under `layout`
        (slot_bits, value_bits, exponent, slots). r and index_base count ciphertexts. Returns (words [C, ct_words],
        statuses [N])."""
        x = np.ascontiguousarray(x)
        dt = scalar_dtype(x)
        N = x.size
        lay = pack_layout(layout)
        C = -(-N // lay.slots) if lay.slots > 0 else 0
        ct = np.empty((C, self.ct_words), dtype=np.uint32)
        st = np.empty(N, dtype=np.int32)
        r_buf, r_stride, r_bytes = None, 0, 0
        if obf_mode == PAI_OBF_GIVEN:
            r_bytes = self.ct_words * 4
            r_buf = np.frombuffer(b"".join(int_to_le(v, r_bytes) for v in r), dtype=np.uint8).copy()
            r_stride = r_bytes
        key = rng_key if rng_key is not None else os.urandom(32)
        self.calls["pai_encrypt_packed"] += 1
        self._chk(self.lib.pai_encrypt_packed(self._h, dt, _ptr(x), N, ctypes.byref(lay), obf_mode,
                                              _ptr(r_buf) if r_buf is not None else None, r_stride, r_bytes, key,
                                              index_base, _ptr(ct), _ptr(st)))
        return ct, st

    def decrypt_packed(self, ct: np.ndarray, layout, N: int):
        """pai_decrypt_packed: the first N values of the packed ciphertexts ct [ceil(N / slots), ct_words]. Returns
        (val float64 [N], mant int64 [N], statuses [N])."""
        ct = np.ascontiguousarray(ct, dtype=np.uint32)
        lay = pack_layout(layout)
        N = int(N)
        C = -(-N // lay.slots) if lay.slots > 0 else 0
        if lay.slots > 0 and (ct.ndim != 2 or ct.shape != (C, self.ct_words)):
            raise ValueError(f"ciphertext buffer shape {ct.shape} does not match ({C}, {self.ct_words})")
        val = np.empty(N, dtype=np.float64)
        mant = np.empty(N, dtype=np.int64)
        st = np.empty(N, dtype=np.int32)
        self.calls["pai_decrypt_packed"] += 1
        self._chk(self.lib.pai_decrypt_packed(self._h, _ptr(ct), ctypes.byref(lay), N, _ptr(val), _ptr(mant), _ptr(st)))
        return val, mant, st

    def pack_ciphertexts(self, ct: np.ndarray, exp: np.ndarray, layout) -> Tuple[np.ndarray, np.ndarray]:
        """pai_pack_ciphertexts: fold the N ordinary ciphertexts ct [N, ct_words] with exponents exp into
        ceil(N / slots) packed ones under `layout`. Returns (words [C, ct_words], statuses [N])."""
        ct = np.ascontiguousarray(ct, dtype=np.uint32)
        exp = np.ascontiguousarray(exp, dtype=np.int32)
        N = exp.size
        self._check_words(ct, exp, N)
        lay = pack_layout(layout)
        C = -(-N // lay.slots) if lay.slots > 0 else 0
        out = np.empty((C, self.ct_words), dtype=np.uint32)
        st = np.empty(N, dtype=np.int32)
        self.calls["pai_pack_ciphertexts"] += 1
        self._chk(self.lib.pai_pack_ciphertexts(self._h, _ptr(ct), _ptr(exp), N, ctypes.byref(lay), _ptr(out), _ptr(st)))
        return out, st

    def repack(self, ct: np.ndarray, layout, group: int) -> np.ndarray:
        """pai_repack: fold the N packed ciphertexts ct [N, ct_words] under `layout`, `group` at a time, into
        ceil(N / group) ciphertexts of layout.slots * group slots. Returns words [C, ct_words]."""
        ct = np.ascontiguousarray(ct, dtype=np.uint32)
        if ct.ndim != 2 or ct.shape[1] != self.ct_words:
            raise ValueError(f"ciphertext buffer shape {ct.shape} does not match (N, {self.ct_words})")
        lay, group, N = pack_layout(layout), int(group), ct.shape[0]
        out = np.empty((-(-N // group) if group > 0 else 0, self.ct_words), dtype=np.uint32)
        self.calls["pai_repack"] += 1
        self._chk(self.lib.pai_repack(self._h, _ptr(ct), N, ctypes.byref(lay), group, _ptr(out)))
        return out

    def add(self, cts: Sequence[np.ndarray], exps: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
        k = len(cts)
        cts = [np.ascontiguousarray(c, dtype=np.uint32) for c in cts]
        exps = [np.ascontiguousarray(e, dtype=np.int32) for e in exps]
        N = exps[0].size
        for c, e in zip(cts, exps):
            self._check_words(c, e, N)
        self.calls["pai_add"] += 1
        ct_ptrs = (ctypes.c_void_p * k)(*[_ptr(c) for c in cts])
        ex_ptrs = (ctypes.c_void_p * k)(*[_ptr(e) for e in exps])
        out = np.empty((N, self.ct_words), dtype=np.uint32)
        oe = np.empty(N, dtype=np.int32)
        self._chk(self.lib.pai_add(self._h, ct_ptrs, ex_ptrs, k, N, _ptr(out), _ptr(oe)))
        return out, oe

    def mul(self, ct: np.ndarray, exp: np.ndarray, x: np.ndarray):
        """Element-wise ct_i (x) x_i (x of size 1: one scalar for every element); returns
        (ciphertext words, exponents, statuses). PaillierEncryptedNumber.__mul__ semantics."""
        ct = np.ascontiguousarray(ct, dtype=np.uint32)
        exp = np.ascontiguousarray(exp, dtype=np.int32)
        x = np.ascontiguousarray(x)
        N = exp.size
        self._check_words(ct, exp, N)
        if x.size not in (1, N):
            raise ValueError("scalar operand must have 1 or N elements")
        self.calls["pai_mul"] += 1
        out = np.empty((N, self.ct_words), dtype=np.uint32)
        oe = np.empty(N, dtype=np.int32)
        st = np.empty(N, dtype=np.int32)
        self._chk(self.lib.pai_mul(self._h, _ptr(ct), _ptr(exp), N, scalar_dtype(x), _ptr(x), 1 if x.size == N and N > 1 else 0,
                                _ptr(out), _ptr(oe), _ptr(st)))
        return out, oe, st

    def add_plain(self, ct: np.ndarray, exp: np.ndarray, x: np.ndarray):
        """Element-wise ct_i (+) x_i (x of size 1: one scalar for every element); returns (ciphertext
        words, exponents, statuses). PaillierEncryptedNumber.__add__(scalar) semantics."""
        ct = np.ascontiguousarray(ct, dtype=np.uint32)
        exp = np.ascontiguousarray(exp, dtype=np.int32)
        x = np.ascontiguousarray(x)
        N = exp.size
        self._check_words(ct, exp, N)
        if x.size not in (1, N):
            raise ValueError("plain operand must have 1 or N elements")
        self.calls["pai_add_plain"] += 1
        out = np.empty((N, self.ct_words), dtype=np.uint32)
        oe = np.empty(N, dtype=np.int32)
        st = np.empty(N, dtype=np.int32)
        self._chk(self.lib.pai_add_plain(self._h, _ptr(ct), _ptr(exp), N, scalar_dtype(x), _ptr(x),
                                      1 if x.size == N and N > 1 else 0, _ptr(out), _ptr(oe), _ptr(st)))
        return out, oe, st

    def segment_add(self, ct: np.ndarray, exp: np.ndarray, index: np.ndarray, seg_off: np.ndarray):
        """Per-segment k-way sums: segment s = ct[index[seg_off[s]:seg_off[s+1]]]. Returns (words [nseg, W],
        exponents [nseg]); an empty segment gives ciphertext 1 and exponent INT32_MIN."""
        ct = np.ascontiguousarray(ct, dtype=np.uint32)
        exp = np.ascontiguousarray(exp, dtype=np.int32)
        index = np.ascontiguousarray(index, dtype=np.int64)
        seg_off = np.ascontiguousarray(seg_off, dtype=np.int64)
        nseg = seg_off.size - 1
        self._check_words(ct, exp, exp.size)
        self.calls["pai_segment_add"] += 1
        out = np.empty((max(nseg, 0), self.ct_words), dtype=np.uint32)
        oe = np.empty(max(nseg, 0), dtype=np.int32)
        if nseg <= 0:
            return out, oe
        self._chk(self.lib.pai_segment_add(self._h, _ptr(ct), _ptr(exp), exp.size, _ptr(index), _ptr(seg_off), nseg,
                                        _ptr(out), _ptr(oe)))
        return out, oe

    def histogram(self, ct: np.ndarray, exp: np.ndarray, bins: np.ndarray, n_bins: int, node=None, n_nodes: int = 1):
        """Per-cell sums of the N ciphertexts over bins [N, F] (uint8 / uint16, rows may be strided) and an optional
        int32 node id per sample (pai_histogram, one call, no index list). Returns (words [n_nodes F n_bins, W],
        exponents, counts int64), cell (v, f, b) at (v F + f) n_bins + b; an empty cell gives ciphertext 1 and exponent
        INT32_MIN. The arguments are the checked ones of cipher_buffer.histogram_args."""
        ct = np.ascontiguousarray(ct, dtype=np.uint32)
        exp = np.ascontiguousarray(exp, dtype=np.int32)
        N = exp.size
        self._check_words(ct, exp, N)
        if bins.ndim != 2 or bins.shape[0] != N or bins.dtype not in (np.uint8, np.uint16):
            raise ValueError("histogram: bins must be a uint8 / uint16 matrix with one row per ciphertext")
        isz = bins.dtype.itemsize
        F = bins.shape[1]
        if N > 1 and F > 0 and (bins.strides[1] != isz or bins.strides[0] % isz or bins.strides[0] < F * isz):
            raise ValueError("histogram: bins must be C-contiguous or row-strided")
        stride = bins.strides[0] // isz if N > 1 and F > 0 else max(F, 1)
        if bins.size and N <= 1:
            bins = np.ascontiguousarray(bins)
        if node is not None:
            node = np.ascontiguousarray(node, dtype=np.int32)
            if node.shape != (N,):
                raise ValueError("histogram: one node id per ciphertext")
        cells = int(n_nodes) * F * int(n_bins)
        self.calls["pai_histogram"] += 1
        out = np.empty((max(cells, 0), self.ct_words), dtype=np.uint32)
        oe = np.empty(max(cells, 0), dtype=np.int32)
        cnt = np.empty(max(cells, 0), dtype=np.int64)
        self._chk(self.lib.pai_histogram(self._h, _ptr(ct), _ptr(exp), N, PAI_BIN_U16 if isz == 2 else PAI_BIN_U8,
                                      _ptr(bins), F, stride, _ptr(node) if node is not None else None, int(n_nodes),
                                      int(n_bins), _ptr(out), _ptr(oe), _ptr(cnt)))
        return out, oe, cnt

    def histogram_sparse(self, ct: np.ndarray, exp: np.ndarray, indptr: np.ndarray, indices: np.ndarray, data: np.ndarray,
                         n_features: int, default_bin: np.ndarray, n_bins: int, node=None, n_nodes: int = 1):
        """histogram over a CSR matrix of bin ids (pai_histogram_sparse, one call): indptr [N + 1], indices (features,
        strictly increasing inside a row) and data (uint8 / uint16 bin ids) of the stored entries, default_bin [F] the
        bin of every entry that is not stored. Returns (words [n_nodes F n_bins, W], exponents, counts int64) laid out
        like histogram; the default cells are T_v - S_{v,f} (include/flexpai.h). The arguments are the checked ones of
        cipher_buffer.histogram_sparse_args."""
        ct = np.ascontiguousarray(ct, dtype=np.uint32)
        exp = np.ascontiguousarray(exp, dtype=np.int32)
        N = exp.size
        self._check_words(ct, exp, N)
        if data.dtype not in (np.uint8, np.uint16):
            raise ValueError("histogram: the stored bin ids must be uint8 or uint16")
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        data = np.ascontiguousarray(data)
        default_bin = np.ascontiguousarray(default_bin, dtype=np.int32)
        F = int(n_features)
        if indptr.shape != (N + 1,) or indices.shape != data.shape or indices.ndim != 1 or default_bin.shape != (F,):
            raise ValueError("histogram: malformed CSR operand")
        if node is not None:
            node = np.ascontiguousarray(node, dtype=np.int32)
            if node.shape != (N,):
                raise ValueError("histogram: one node id per ciphertext")
        cells = int(n_nodes) * F * int(n_bins)
        self.calls["pai_histogram_sparse"] += 1
        out = np.empty((max(cells, 0), self.ct_words), dtype=np.uint32)
        oe = np.empty(max(cells, 0), dtype=np.int32)
        cnt = np.empty(max(cells, 0), dtype=np.int64)
        self._chk(self.lib.pai_histogram_sparse(self._h, _ptr(ct), _ptr(exp), N, _ptr(indptr), _ptr(indices),
                                             PAI_BIN_U16 if data.dtype.itemsize == 2 else PAI_BIN_U8, _ptr(data), F,
                                             _ptr(default_bin), _ptr(node) if node is not None else None, int(n_nodes),
                                             int(n_bins), _ptr(out), _ptr(oe), _ptr(cnt)))
        return out, oe, cnt

    def cumsum(self, ct: np.ndarray, exp: np.ndarray, outer: int, L: int, inner: int, reverse: bool = False):
        """Prefix sums along the middle axis of the C-contiguous [outer, L, inner] array of ciphertexts (pai_cumsum;
        reverse: suffix sums). Returns (words [outer L inner, W], exponents); entries with exponent INT32_MIN are
        skipped, and a prefix of such entries only is ciphertext 1 with exponent INT32_MIN."""
        ct = np.ascontiguousarray(ct, dtype=np.uint32)
        exp = np.ascontiguousarray(exp, dtype=np.int32)
        outer, L, inner = int(outer), int(L), int(inner)
        if min(outer, L, inner) < 0 or outer * L * inner != exp.size:
            raise ValueError("cumsum: outer * L * inner must be the number of ciphertexts")
        N = exp.size
        self._check_words(ct, exp, N)
        self.calls["pai_cumsum"] += 1
        out = np.empty((N, self.ct_words), dtype=np.uint32)
        oe = np.empty(N, dtype=np.int32)
        self._chk(self.lib.pai_cumsum(self._h, _ptr(ct), _ptr(exp), outer, L, inner, PAI_SCAN_REVERSE if reverse else 0,
                                   _ptr(out), _ptr(oe)))
        return out, oe

    def segment_dot(self, ct: np.ndarray, exp: np.ndarray, index: np.ndarray, seg_off: np.ndarray, x: np.ndarray):
        """Per-segment weighted sums: segment s = sum over t in [seg_off[s], seg_off[s+1]) of ct[index[t]] (x) x[t]
        (x: one float32 / float64 / int64 scalar per entry). Returns (words [nseg, W], exponents [nseg], statuses
        [nnz], pai_mul's); an empty segment gives ciphertext 1 and exponent INT32_MIN."""
        ct = np.ascontiguousarray(ct, dtype=np.uint32)
        exp = np.ascontiguousarray(exp, dtype=np.int32)
        index = np.ascontiguousarray(index, dtype=np.int64)
        seg_off = np.ascontiguousarray(seg_off, dtype=np.int64)
        x = np.ascontiguousarray(x)
        nseg = seg_off.size - 1
        self._check_words(ct, exp, exp.size)
        if x.ndim != 1 or x.size != index.size:
            raise ValueError("segment_dot: one scalar per index entry")
        if nseg >= 0 and seg_off.size and int(seg_off[-1]) != index.size:
            raise ValueError("segment_dot: seg_off[-1] must equal the number of entries")
        self.calls["pai_segment_dot"] += 1
        out = np.empty((max(nseg, 0), self.ct_words), dtype=np.uint32)
        oe = np.empty(max(nseg, 0), dtype=np.int32)
        st = np.zeros(index.size, dtype=np.int32)
        if nseg <= 0:
            return out, oe, st
        self._chk(self.lib.pai_segment_dot(self._h, _ptr(ct), _ptr(exp), exp.size, _ptr(index), _ptr(seg_off), nseg,
                                        scalar_dtype(x), _ptr(x), _ptr(out), _ptr(oe), _ptr(st)))
        return out, oe, st

    def matmul(self, ct: np.ndarray, exp: np.ndarray, m: int, K: int, x: np.ndarray, d: int):
        """(m x K encrypted) @ (K x d plain) -> (m d ciphertext words, m d exponents), row-major."""
        ct = np.ascontiguousarray(ct, dtype=np.uint32)
        exp = np.ascontiguousarray(exp, dtype=np.int32)
        x = np.ascontiguousarray(x)
        if exp.size != m * K or x.size != K * d:
            raise ValueError("matmul: shape mismatch")
        self._check_words(ct, exp, m * K)
        self.calls["pai_matmul"] += 1
        out = np.empty((m * d, self.ct_words), dtype=np.uint32)
        oe = np.empty(m * d, dtype=np.int32)
        self._chk(self.lib.pai_matmul(self._h, _ptr(ct), _ptr(exp), m, K, scalar_dtype(x), _ptr(x), d, _ptr(out), _ptr(oe)))
        return out, oe

    def decrypt(self, ct: np.ndarray, exp: np.ndarray, want_raw: bool = False):
        ct = np.ascontiguousarray(ct, dtype=np.uint32)
        exp = np.ascontiguousarray(exp, dtype=np.int32)
        N = exp.size
        self._check_words(ct, exp, N)
        self.calls["pai_decrypt"] += 1
        val = np.empty(N, dtype=np.float64)
        mant = np.empty(N, dtype=np.int64)
        st = np.empty(N, dtype=np.int32)
        raw = np.empty((N, self.pt_words), dtype=np.uint32) if want_raw else None
        self._chk(self.lib.pai_decrypt(self._h, _ptr(ct), _ptr(exp), N, _ptr(val), _ptr(mant), _ptr(st),
                                    _ptr(raw) if raw is not None else None))
        return val, mant, st, raw


class PackLayoutC(ctypes.Structure):
    """pai_pack_layout (include/flexpai.h)."""
    _fields_ = [("slot_bits", ctypes.c_int32), ("value_bits", ctypes.c_int32), ("exponent", ctypes.c_int32),
                ("slots", ctypes.c_int32)]


def pack_layout(layout) -> PackLayoutC:
    """A pai_pack_layout from (slot_bits, value_bits, exponent, slots) or from an object with those attributes."""
    if isinstance(layout, PackLayoutC):
        return layout
    if isinstance(layout, (tuple, list)):
        sb, vb, e, k = layout
    else:
        sb, vb, e, k = layout.slot_bits, layout.value_bits, layout.exponent, layout.slots
    return PackLayoutC(int(sb), int(vb), int(e), int(k))


def scalar_dtype(x: np.ndarray) -> int:
    if x.dtype == np.float32:
        return PAI_F32
    if x.dtype == np.float64:
        return PAI_F64
    if x.dtype == np.int64:
        return PAI_I64
    raise TypeError(f"unsupported dtype {x.dtype}")


try:                                        # the package's C conversions (csrc/hostgmp.c), when built
    from .._gmp import ints_to_words as _c_ints_to_words, words_to_ints as _c_words_to_ints
except ImportError:                         # pragma: no cover - build() always builds it
    _c_ints_to_words = _c_words_to_ints = None


def words_to_ints(words: np.ndarray):
    """[N, W] little-endian uint32 words -> list of Python ints."""
    w = np.ascontiguousarray(words, dtype="<u4")
    if w.ndim != 2:
        w = w.reshape(len(w), -1)
    if _c_words_to_ints is not None and w.size:
        return _c_words_to_ints(w, w.shape[1])
    b = w.tobytes()
    step = w.shape[1] * 4
    return [int.from_bytes(b[i * step:(i + 1) * step], "little") for i in range(w.shape[0])]


def ints_to_words(vals, nwords: int) -> np.ndarray:
    vals = list(vals)
    if _c_ints_to_words is not None:
        buf = _c_ints_to_words(vals, nwords)
    else:
        nbytes = nwords * 4
        buf = b"".join(int(v).to_bytes(nbytes, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u4").reshape(len(vals), nwords).copy()


# ---------------------------------------------------------------- key generation: the prime search on the device
PRIME_BITS = (256, 512, 1024, 2048)      # the sizes k_mr_w is built for (csrc/kernels_prime.hpp)
PAI_PRIME_OVERFLOW = 1
_prime_stats = collections.Counter()


def prime_stats() -> dict:
    """Which path the prime searches of this process took: device searches (starts answered by pai_next_prime), the
    windows those used, host fallbacks (starts an eligible call handed back to _bigint.next_prime)."""
    return {k: _prime_stats[k] for k in ("device_searches", "windows", "host_fallbacks")}


def count_host_fallback(n: int = 1) -> None:
    _prime_stats["host_fallbacks"] += n


def prime_sieve(x: int, bits: int, window: int = 0):
    """pai_debug_prime_sieve: the offsets the device search would test in (x, x + window], or None when the window
    crosses 2^bits. Host only."""
    lib = load_library()
    nbytes = bits // 8
    cap = (window or 4 * bits) // 2 + 1
    out = np.zeros(cap, dtype=np.uint32)
    cnt = ctypes.c_size_t()
    rc = lib.pai_debug_prime_sieve(bits, int_to_le(x, nbytes), nbytes, window, _ptr(out), cap, ctypes.byref(cnt))
    if rc == PAI_PRIME_OVERFLOW:
        return None
    _check(rc, lib)
    return [int(v) for v in out[:cnt.value]]


def prime_test(cands, bits: int, bases, device: int = 0) -> np.ndarray:
    """pai_prime_test: the [len(cands), len(bases)] uint8 matrix of strong-probable-prime verdicts (k_mr_w)."""
    global _runtime_started
    lib = load_library()
    cands = list(cands)
    nbytes = bits // 8
    buf = b"".join(int_to_le(c, nbytes) for c in cands)
    b = np.ascontiguousarray(bases, dtype=np.uint32)
    out = np.zeros((len(cands), b.size), dtype=np.uint8)
    _runtime_started = True
    _check(lib.pai_prime_test(device, bits, buf, nbytes, len(cands), _ptr(b), b.size, _ptr(out)), lib)
    return out


def next_prime_batch(starts, bits: int, window: int = 0, device: int = 0):
    """pai_next_prime: for every start (bit `bits - 1` set) the smallest prime above it, as _bigint.next_prime finds
    it, searched on the device in one batch. Returns (primes, passes): primes[i] is None, and passes[i] is -1, where
    the start's window would cross 2^bits (the caller searches that one on the host)."""
    global _runtime_started
    lib = load_library()
    starts = list(starts)
    nbytes = bits // 8
    buf = b"".join(int_to_le(s, nbytes) for s in starts)
    out = ctypes.create_string_buffer(nbytes * len(starts))
    passes = np.zeros(len(starts), dtype=np.int32)
    _runtime_started = True
    rc = lib.pai_next_prime(device, bits, buf, nbytes, len(starts), window, out, _ptr(passes))
    if rc != PAI_PRIME_OVERFLOW:
        _check(rc, lib)
    raw = out.raw
    primes = [None if passes[i] < 0 else int.from_bytes(raw[i * nbytes:(i + 1) * nbytes], "little")
              for i in range(len(starts))]
    _prime_stats["device_searches"] += sum(p is not None for p in primes)
    _prime_stats["windows"] += int(passes[passes > 0].sum())
    return primes, [int(v) for v in passes]


def prime_last_times():
    """(pass-1 ms, pass-2 ms, pass-1 launches, pass-2 launches) of this thread's last next_prime_batch."""
    a, b = ctypes.c_float(), ctypes.c_float()
    c, d = ctypes.c_int(), ctypes.c_int()
    _check(load_library().pai_prime_last_times(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
    return a.value, b.value, c.value, d.value
