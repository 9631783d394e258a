// Key generation's prime search (kernels_prime.hpp): the sieve, the two Miller-Rabin passes and the C entry points
// pai_prime_test, pai_next_prime, pai_prime_last_times and pai_debug_prime_sieve. Context-free: a key does not exist
// yet. Each device keeps one stream, two events and one scratch buffer for these calls, under one mutex (creating and
// releasing them per call was measured: 3.6 ms per call, three times a 1024-bit keypair's whole search).
#include "engine_prime.hpp"

#include <map>
#include <mutex>
#include <string>

#include "flexpai.h"

namespace fpai {
int set_error(int code, const char* msg);   // flexpai.hip

hipError_t mr_launch(int bits, const prime::Params& p, hipStream_t st) {
  const long long blocks = (p.nwork + prime::GPW - 1) / prime::GPW;
  const int gx = (int)std::min<long long>(blocks, 1ll << 20);
  if (bits == 256) hipLaunchKernelGGL((prime::k_mr_w<10>), dim3(gx), dim3(prime::BLOCK_W), 0, st, p);
  else if (bits == 512) hipLaunchKernelGGL((prime::k_mr_w<19>), dim3(gx), dim3(prime::BLOCK_W), 0, st, p);
  else if (bits == 1024) hipLaunchKernelGGL((prime::k_mr_w<37>), dim3(gx), dim3(prime::BLOCK_W), 0, st, p);
  else if (bits == 2048) hipLaunchKernelGGL((prime::k_mr_w<74>), dim3(gx), dim3(prime::BLOCK_W), 0, st, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

const std::vector<uint32_t>& odd_small_primes() {
  static const std::vector<uint32_t> v = [] {
    std::vector<uint32_t> a = small_primes(PRIME_SIEVE_BOUND);
    a.erase(a.begin());   // 2
    return a;
  }();
  return v;
}

std::vector<uint32_t> prime_residues(const HBig& x) {
  const std::vector<uint32_t>& ps = odd_small_primes();
  std::vector<uint32_t> r(ps.size());
  Mpz v(x);
  for (size_t i = 0; i < ps.size(); ++i) r[i] = (uint32_t)mpz_fdiv_ui(v.v, ps[i]);
  return r;
}

void prime_sieve_window(const HBig& x, const std::vector<uint32_t>& residues, uint32_t lo, uint32_t window,
                        std::vector<uint32_t>& offsets) {
  const std::vector<uint32_t>& ps = odd_small_primes();
  std::vector<uint8_t> comp((size_t)window + 1, 0);   // comp[k]: x + lo + k has a small factor
  for (size_t i = 0; i < ps.size(); ++i) {
    const uint64_t p = ps[i];
    const uint64_t r = (residues[i] + (uint64_t)lo + 1) % p;   // (x + lo + 1) mod p
    for (uint64_t k = 1 + (p - r) % p; k <= window; k += p) comp[k] = 1;
  }
  const uint32_t x_odd = x.is_odd() ? 1u : 0u;
  for (uint32_t k = 1; k <= window; ++k) {
    const uint32_t off = lo + k;
    if (((x_odd + off) & 1u) && !comp[k]) offsets.push_back(off);
  }
}

}  // namespace fpai

using namespace fpai;

namespace {

#define PHIPCHK(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) return set_error(PAI_ERR_HIP, (std::string(#expr ": ") + hipGetErrorString(_e)).c_str()); \
  } while (0)

struct PrimeDev {   // a device's state for these calls, kept for the life of the process
  int device = 0;
  hipStream_t st = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  void* buf = nullptr;
  size_t bytes = 0;
};
std::mutex g_mu;                     // held for the whole of a device call
std::map<int, PrimeDev> g_dev;
PrimeDev& dev_state(int device) {
  PrimeDev& d = g_dev[device];
  d.device = device;
  return d;
}
thread_local float g_ms[2] = {0.f, 0.f};   // the last pai_next_prime: kernel time of pass 1, of pass 2
thread_local int g_launches[2] = {0, 0};

bool bits_ok(int bits) { return bits == 256 || bits == 512 || bits == 1024 || bits == 2048; }
size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
uint32_t default_window(int bits) { return 4u * (uint32_t)bits; }

// one launch: verdict[w] for the work items (start index, offset, base) over the starts' words x [nstarts][bits / 32]
int run_items(PrimeDev& d, int bits, const std::vector<uint32_t>& x, int nstarts, const std::vector<uint32_t>& work,
              std::vector<uint8_t>& verdict, float* ms) {
  const size_t nwork = work.size() / 3;
  verdict.assign(nwork, 0);
  if (nwork == 0) return 0;
  PHIPCHK(hipSetDevice(d.device));
  if (!d.st) PHIPCHK(hipStreamCreateWithFlags(&d.st, hipStreamNonBlocking));
  for (int i = 0; i < 2; ++i)
    if (!d.ev[i]) PHIPCHK(hipEventCreate(&d.ev[i]));
  const size_t xb = align16(x.size() * 4), wb = align16(work.size() * 4), vb = align16(nwork);
  if (xb + wb + vb > d.bytes) {
    if (d.buf) PHIPCHK(hipFree(d.buf));
    d.buf = nullptr;
    d.bytes = 0;
    PHIPCHK(hipMalloc(&d.buf, xb + wb + vb));
    d.bytes = xb + wb + vb;
  }
  uint8_t* b = (uint8_t*)d.buf;
  PHIPCHK(hipMemcpyAsync(b, x.data(), x.size() * 4, hipMemcpyHostToDevice, d.st));
  PHIPCHK(hipMemcpyAsync(b + xb, work.data(), work.size() * 4, hipMemcpyHostToDevice, d.st));
  prime::Params p;
  p.x = (const uint32_t*)b;
  p.work = (const uint32_t*)(b + xb);
  p.nwork = (long long)nwork;
  p.nstarts = nstarts;
  p.verdict = b + xb + wb;
  PHIPCHK(hipEventRecord(d.ev[0], d.st));
  PHIPCHK(mr_launch(bits, p, d.st));
  PHIPCHK(hipEventRecord(d.ev[1], d.st));
  PHIPCHK(hipMemcpyAsync(verdict.data(), p.verdict, nwork, hipMemcpyDeviceToHost, d.st));
  PHIPCHK(hipStreamSynchronize(d.st));
  if (ms) {
    float t = 0.f;
    PHIPCHK(hipEventElapsedTime(&t, d.ev[0], d.ev[1]));
    *ms += t;
  }
  return 0;
}

// x + off past 2^bits - 1
bool crosses_width(const HBig& x, uint64_t off, int bits) { return add(x, HBig(off)).bits() > (size_t)bits; }

struct Search {
  HBig x;
  std::vector<uint32_t> res;    // x mod the sieve's primes
  uint32_t lo = 0;              // the windows so far end at x + lo
  int passes = 0;
  bool done = false, overflow = false;
  std::vector<uint32_t> cand;   // the current window's survivors of pass 1
  size_t next = 0;
  uint32_t found = 0;
};

}  // namespace

int pai_debug_prime_sieve(int bits, const uint8_t* x_le, size_t bytes, uint32_t window, uint32_t* offsets_out,
                          size_t max_out, size_t* count) {
  if (!bits_ok(bits) || !x_le || !count || (max_out && !offsets_out) || window > (1u << 24))
    return set_error(PAI_ERR_ARG, "pai_debug_prime_sieve: bad arguments");
  const HBig x = HBig::from_le_bytes(x_le, bytes);
  if (x.bits() != (size_t)bits) return set_error(PAI_ERR_ARG, "pai_debug_prime_sieve: the start must have bit `bits - 1` set");
  if (!window) window = default_window(bits);
  *count = 0;
  if (crosses_width(x, window, bits)) return PAI_PRIME_OVERFLOW;
  std::vector<uint32_t> offs;
  prime_sieve_window(x, prime_residues(x), 0, window, offs);
  *count = offs.size();
  for (size_t i = 0; i < std::min(max_out, offs.size()); ++i) offsets_out[i] = offs[i];
  return 0;
}

int pai_prime_test(int device, int bits, const uint8_t* cands_le, size_t cand_bytes, size_t ncand, const uint32_t* bases_u32,
                   size_t nbases, uint8_t* verdict_u8) {
  if (!bits_ok(bits) || !cands_le || !bases_u32 || !verdict_u8 || ncand == 0 || nbases == 0 || cand_bytes == 0 ||
      ncand > (1u << 20) || nbases > (1u << 12))
    return set_error(PAI_ERR_ARG, "pai_prime_test: bad arguments");
  const int xw = bits / 32;
  std::vector<uint32_t> x(ncand * xw), work;
  for (size_t i = 0; i < ncand; ++i) {
    const HBig c = HBig::from_le_bytes(cands_le + i * cand_bytes, cand_bytes);
    if (c.bits() != (size_t)bits || !c.is_odd())
      return set_error(PAI_ERR_ARG, "pai_prime_test: a candidate must be odd with bit `bits - 1` set");
    const std::vector<uint32_t> w = c.words(xw);
    std::copy(w.begin(), w.end(), x.begin() + i * xw);
  }
  work.reserve(ncand * nbases * 3);
  for (size_t i = 0; i < ncand; ++i)
    for (size_t j = 0; j < nbases; ++j) {
      work.push_back((uint32_t)i);
      work.push_back(0u);
      work.push_back(bases_u32[j]);
    }
  std::lock_guard<std::mutex> lk(g_mu);
  PrimeDev& d = dev_state(device);
  std::vector<uint8_t> v;
  if (int rc = run_items(d, bits, x, (int)ncand, work, v, nullptr)) return rc;
  std::copy(v.begin(), v.end(), verdict_u8);
  return 0;
}

int pai_next_prime(int device, int bits, const uint8_t* starts_le, size_t start_bytes, size_t nstarts, uint32_t window,
                   uint8_t* out_le, int32_t* passes_out) {
  if (!bits_ok(bits) || !starts_le || !out_le || nstarts == 0 || nstarts > 4096 || start_bytes * 8 < (size_t)bits ||
      window > (1u << 24))
    return set_error(PAI_ERR_ARG, "pai_next_prime: bad arguments");
  if (!window) window = default_window(bits);
  const int xw = bits / 32;
  std::vector<Search> ss(nstarts);
  std::vector<uint32_t> x(nstarts * xw);
  for (size_t i = 0; i < nstarts; ++i) {
    ss[i].x = HBig::from_le_bytes(starts_le + i * start_bytes, start_bytes);
    if (ss[i].x.bits() != (size_t)bits) return set_error(PAI_ERR_ARG, "pai_next_prime: a start must have bit `bits - 1` set");
    ss[i].res = prime_residues(ss[i].x);
    const std::vector<uint32_t> w = ss[i].x.words(xw);
    std::copy(w.begin(), w.end(), x.begin() + i * xw);
  }
  const std::vector<uint32_t>& bases = odd_small_primes();   // 3, 5, 7, ...: base 3 in pass 1, the next 39 in pass 2
  std::lock_guard<std::mutex> lk(g_mu);
  PrimeDev& d = dev_state(device);
  g_ms[0] = g_ms[1] = 0.f;
  g_launches[0] = g_launches[1] = 0;
  std::vector<uint32_t> work;
  std::vector<uint8_t> v;
  for (;;) {
    // pass 1: every sieve survivor of the next window of every start that has no candidate left, against base 3
    work.clear();
    std::vector<std::pair<size_t, size_t>> span(nstarts, {0, 0});   // [first, last) work item of a start
    for (size_t i = 0; i < nstarts; ++i) {
      Search& s = ss[i];
      if (s.done || s.overflow || s.next < s.cand.size()) continue;
      if ((uint64_t)s.lo + window > 0xFFFFFFFFull || crosses_width(s.x, (uint64_t)s.lo + window, bits)) {
        s.overflow = true;
        continue;
      }
      std::vector<uint32_t> offs;
      prime_sieve_window(s.x, s.res, s.lo, window, offs);
      s.lo += window;
      s.passes += 1;
      span[i].first = work.size() / 3;
      for (uint32_t off : offs) {
        work.push_back((uint32_t)i);
        work.push_back(off);
        work.push_back(bases[0]);
      }
      span[i].second = work.size() / 3;
    }
    if (!work.empty()) {
      if (int rc = run_items(d, bits, x, (int)nstarts, work, v, &g_ms[0])) return rc;
      g_launches[0] += 1;
      for (size_t i = 0; i < nstarts; ++i) {
        if (span[i].first == span[i].second) continue;
        ss[i].cand.clear();
        ss[i].next = 0;
        for (size_t w = span[i].first; w < span[i].second; ++w)
          if (v[w]) ss[i].cand.push_back(work[w * 3 + 1]);
      }
    }
    // pass 2: each start's smallest remaining candidate against the other 39 bases, until one holds or none is left
    for (;;) {
      work.clear();
      std::vector<size_t> who;
      for (size_t i = 0; i < nstarts; ++i) {
        Search& s = ss[i];
        if (s.done || s.overflow || s.next >= s.cand.size()) continue;
        who.push_back(i);
        for (int b = 1; b < PRIME_MR_BASES; ++b) {
          work.push_back((uint32_t)i);
          work.push_back(s.cand[s.next]);
          work.push_back(bases[b]);
        }
      }
      if (who.empty()) break;
      if (int rc = run_items(d, bits, x, (int)nstarts, work, v, &g_ms[1])) return rc;
      g_launches[1] += 1;
      for (size_t k = 0; k < who.size(); ++k) {
        Search& s = ss[who[k]];
        bool all = true;
        for (int b = 0; b < PRIME_MR_BASES - 1; ++b) all = all && v[k * (PRIME_MR_BASES - 1) + b];
        if (all) {
          s.done = true;
          s.found = s.cand[s.next];
        } else {
          s.next += 1;
        }
      }
    }
    bool open = false;
    for (const Search& s : ss) open = open || !(s.done || s.overflow);
    if (!open) break;
  }
  int rc = 0;
  for (size_t i = 0; i < nstarts; ++i) {
    const Search& s = ss[i];
    uint8_t* o = out_le + i * start_bytes;
    std::fill(o, o + start_bytes, (uint8_t)0);
    if (s.overflow) {
      if (passes_out) passes_out[i] = -1;
      rc = PAI_PRIME_OVERFLOW;
      continue;
    }
    const HBig c = add(s.x, HBig((uint64_t)s.found));
    for (size_t k = 0; k < c.w.size() * 4 && k < start_bytes; ++k) o[k] = (uint8_t)(c.w[k / 4] >> (8 * (k % 4)));
    if (passes_out) passes_out[i] = s.passes;
  }
  return rc;
}

int pai_prime_last_times(float* pass1_ms, float* pass2_ms, int* pass1_launches, int* pass2_launches) {
  if (pass1_ms) *pass1_ms = g_ms[0];
  if (pass2_ms) *pass2_ms = g_ms[1];
  if (pass1_launches) *pass1_launches = g_launches[0];
  if (pass2_launches) *pass2_launches = g_launches[1];
  return 0;
}
