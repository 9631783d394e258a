// Device-resident ciphertext buffers: the launches of kernels_res.hpp and the context-free C entry points
// pai_dev_alloc, pai_dev_free, pai_dev_upload, pai_dev_download, pai_dev_copy, pai_dev_io_stats and
// pai_dev_release_staging. The memory belongs
// to a device, not to a context: the Python layer drops contexts (LRU) while buffers they filled live on. Each device
// keeps one copy stream, two pinned staging slots and two events for the transfers, under one mutex.
#include "kernels_res.hpp"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>

#include "flexpai.h"

#ifndef FLEXPAI_XCHECK
#define FLEXPAI_XCHECK 0
#endif

namespace fpai {
int set_error(int code, const char* msg);                   // flexpai.hip
hipError_t shared_dev_malloc(void** p, size_t bytes);       // flexpai.hip: dev_malloc (gives the table pool back first)
void shared_par_copy(void* dst, const void* src, size_t bytes);   // flexpai.hip: par_copy (at most 16 host threads)

static int res_grid(long long items, int cus) {
  const long long want = (items + RES_BLOCK - 1) / RES_BLOCK;
  return (int)std::max<long long>(1, std::min<long long>(want, 8ll * std::max(cus, 1)));
}

hipError_t take_launch(const TakeParams& p, int cus, hipStream_t st) {
  const bool wide = p.W % 4 == 0 && ((uintptr_t)p.in % 16 == 0) && ((uintptr_t)p.out % 16 == 0);
  if (wide) hipLaunchKernelGGL(k_take<4>, dim3(res_grid(p.M * (p.W / 4), cus)), dim3(RES_BLOCK), 0, st, p);
  else hipLaunchKernelGGL(k_take<1>, dim3(res_grid(p.M * p.W, cus)), dim3(RES_BLOCK), 0, st, p);
  return hipGetLastError();
}

hipError_t check_below_launch(const CheckBelowParams& p, int cus, hipStream_t st) {
  hipLaunchKernelGGL(k_check_below, dim3(res_grid(p.N, cus)), dim3(RES_BLOCK), 0, st, p);
  return hipGetLastError();
}

hipError_t check_idx_launch(const CheckIdxParams& p, int cus, hipStream_t st) {
  hipLaunchKernelGGL(k_check_idx, dim3(res_grid(std::max(p.total, p.nseg + 1), cus)), dim3(RES_BLOCK), 0, st, p);
  return hipGetLastError();
}

hipError_t seg_offsets_launch(const SegPlanParams& p, hipStream_t st) {
  hipLaunchKernelGGL(k_seg_offsets, dim3(1), dim3(SEGPLAN_BLOCK), 0, st, p);
  return hipGetLastError();
}

hipError_t seg_rows_launch(const SegRowsParams& p, int cus, hipStream_t st) {
  hipLaunchKernelGGL(k_seg_rows, dim3(res_grid(p.rows * SEGPLAN_C, cus)), dim3(RES_BLOCK), 0, st, p);
  return hipGetLastError();
}

}  // namespace fpai

namespace {

constexpr size_t RES_SLOT_MAX = (size_t)64 << 20;   // bytes per pinned staging slot, as PIN_SLOT_MAX of the host calls

struct DevIo {
  hipStream_t st = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  void* pin[2] = {nullptr, nullptr};
  size_t pin_bytes = 0;
};
std::mutex g_io_mu;
std::map<int, DevIo> g_io;
std::atomic<uint64_t> g_h2d{0}, g_d2h{0};

int hip_fail(const char* what, hipError_t e) {
  return fpai::set_error(PAI_ERR_HIP, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}
#define RESCHK(expr)                                   \
  do {                                                 \
    hipError_t _e = (expr);                            \
    if (_e != hipSuccess) return hip_fail(#expr, _e);  \
  } while (0)

// Waits for the copy stream when a transfer leaves its scope, on the error paths too: no copy stays in flight into or
// out of a pinned slot after the call has returned.
struct Drain {
  hipStream_t st;
  ~Drain() { (void)hipStreamSynchronize(st); }
};

// Slot size of a transfer of `bytes`; the test build's $FLEXPAI_RES_SLOT (bytes) shrinks it so that small arrays span
// several slots.
size_t slot_for(size_t bytes) {
  size_t slot = RES_SLOT_MAX;
#if FLEXPAI_XCHECK
  if (const char* e = getenv("FLEXPAI_RES_SLOT")) {
    const unsigned long long v = strtoull(e, nullptr, 10);
    if (v > 0) slot = (size_t)v;
  }
#endif
  return std::min(slot, std::max<size_t>(bytes, 1));
}

// The device's stream, events and pinned slots of at least `slot` bytes. Caller holds g_io_mu.
int io_state(int device, size_t slot, DevIo** out) {
  RESCHK(hipSetDevice(device));
  DevIo& io = g_io[device];
  if (!io.st) RESCHK(hipStreamCreateWithFlags(&io.st, hipStreamNonBlocking));
  for (hipEvent_t& e : io.ev)
    if (!e) RESCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  if (slot > io.pin_bytes) {
    for (void*& p : io.pin) {
      if (p) RESCHK(hipHostFree(p));
      p = nullptr;
    }
    io.pin_bytes = 0;
    for (void*& p : io.pin) RESCHK(hipHostMalloc(&p, slot, hipHostMallocDefault));
    io.pin_bytes = slot;
  }
  *out = &io;
  return 0;
}

}  // namespace

int pai_dev_alloc(int device, size_t bytes, void** d_out) {
  if (!d_out) return fpai::set_error(PAI_ERR_ARG, "pai_dev_alloc: null output");
  *d_out = nullptr;
  RESCHK(hipSetDevice(device));
  RESCHK(fpai::shared_dev_malloc(d_out, std::max<size_t>(bytes, 16)));
  return 0;
}

int pai_dev_free(int device, void* d) {
  if (!d) return 0;
  RESCHK(hipSetDevice(device));
  RESCHK(hipDeviceSynchronize());   // queued kernels may still read the block
  RESCHK(hipFree(d));
  return 0;
}

int pai_dev_upload(int device, void* d_dst, const void* src, size_t bytes) {
  if (bytes == 0) return 0;
  if (!d_dst || !src) return fpai::set_error(PAI_ERR_ARG, "pai_dev_upload: null buffer");
  std::lock_guard<std::mutex> lk(g_io_mu);
  const size_t slot = slot_for(bytes);
  DevIo* io;
  int rc = io_state(device, slot, &io);
  if (rc) return rc;
  RESCHK(hipDeviceSynchronize());   // whatever was queued on the destination is done before it is overwritten
  Drain drain{io->st};
  const size_t nch = (bytes + slot - 1) / slot;
  fpai::shared_par_copy(io->pin[0], src, std::min(slot, bytes));
  for (size_t i = 0; i < nch; ++i) {
    const size_t off = i * slot, n = std::min(slot, bytes - off);
    RESCHK(hipMemcpyAsync((char*)d_dst + off, io->pin[i & 1], n, hipMemcpyHostToDevice, io->st));
    RESCHK(hipEventRecord(io->ev[i & 1], io->st));
    if (i + 1 < nch) {   // fill the other slot while this one crosses PCIe; its previous chunk (i - 1) must have left
      if (i >= 1) RESCHK(hipEventSynchronize(io->ev[(i + 1) & 1]));
      const size_t off1 = off + slot;
      fpai::shared_par_copy(io->pin[(i + 1) & 1], (const char*)src + off1, std::min(slot, bytes - off1));
    }
  }
  RESCHK(hipStreamSynchronize(io->st));
  g_h2d += bytes;
  return 0;
}

int pai_dev_download(int device, void* dst, const void* d_src, size_t bytes) {
  if (bytes == 0) return 0;
  if (!dst || !d_src) return fpai::set_error(PAI_ERR_ARG, "pai_dev_download: null buffer");
  std::lock_guard<std::mutex> lk(g_io_mu);
  const size_t slot = slot_for(bytes);
  DevIo* io;
  int rc = io_state(device, slot, &io);
  if (rc) return rc;
  RESCHK(hipDeviceSynchronize());   // the kernels that write the source are done
  Drain drain{io->st};
  const size_t nch = (bytes + slot - 1) / slot;
  auto d2h = [&](size_t i) -> int {
    const size_t off = i * slot, n = std::min(slot, bytes - off);
    RESCHK(hipMemcpyAsync(io->pin[i & 1], (const char*)d_src + off, n, hipMemcpyDeviceToHost, io->st));
    RESCHK(hipEventRecord(io->ev[i & 1], io->st));
    return 0;
  };
  if ((rc = d2h(0))) return rc;
  for (size_t i = 0; i < nch; ++i) {
    if (i + 1 < nch && (rc = d2h(i + 1))) return rc;   // its slot's previous chunk (i - 1) is consumed
    const size_t off = i * slot, n = std::min(slot, bytes - off);
    RESCHK(hipEventSynchronize(io->ev[i & 1]));
    fpai::shared_par_copy((char*)dst + off, io->pin[i & 1], n);
  }
  g_d2h += bytes;
  return 0;
}

int pai_dev_copy(int device, void* d_dst, const void* d_src, size_t bytes) {
  if (bytes == 0) return 0;
  if (!d_dst || !d_src) return fpai::set_error(PAI_ERR_ARG, "pai_dev_copy: null buffer");
  RESCHK(hipSetDevice(device));
  // on the null stream, where the Python layer queues its *_dev calls: ordered after the kernels that wrote the source
  // and before those that read the destination, with no wait on the host
  RESCHK(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, nullptr));
  return 0;
}

int pai_dev_release_staging(void) {
  std::lock_guard<std::mutex> lk(g_io_mu);
  for (auto& kv : g_io) {
    DevIo& io = kv.second;
    RESCHK(hipSetDevice(kv.first));
    if (io.st) RESCHK(hipStreamSynchronize(io.st));
    for (void*& p : io.pin) {
      if (p) RESCHK(hipHostFree(p));
      p = nullptr;
    }
    io.pin_bytes = 0;
    for (hipEvent_t& e : io.ev) {
      if (e) RESCHK(hipEventDestroy(e));
      e = nullptr;
    }
    if (io.st) RESCHK(hipStreamDestroy(io.st));
    io.st = nullptr;
  }
  return 0;
}

int pai_dev_io_stats(uint64_t* h2d_bytes, uint64_t* d2h_bytes) {
  if (h2d_bytes) *h2d_bytes = g_h2d.load();
  if (d2h_bytes) *d2h_bytes = g_d2h.load();
  return 0;
}
