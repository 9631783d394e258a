// flexpai: host context + C ABI for the MI355X Paillier engine (see include/flexpai.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <sys/random.h>
#include <thread>
#include <array>
#include <vector>
#include <optional>

#include "flexpai.h"
#include "host_bignum.hpp"
#include "table_arena.hpp"
#include "kernels.hpp"
#include "kernels_crt.hpp"
#include "engine_dec.hpp"
#include "engine_lane.hpp"
#include "engine_fb.hpp"
#include "engine_fbp.hpp"
#include "engine_fbs.hpp"

// FLEXPAI_XCHECK (the test-only library libflexpai_xcheck.so, __graft_entry__.build): the kernel generations the
// pair kernels replaced -- k_fbgp, k_pfb, k_fbp (k_fb/k_fb_fin, k_fbg and the 2S-limb k_dec_* / k_crt_b were retired in
// round 6) -- and k_debug, selected by $FLEXPAI_SGP=0 / $FLEXPAI_FBS=0 ($FLEXPAI_PAIR=0: the group-engine decryption and
// the public-key encryption kernels of the product), so that the tests can cross-check the shipping
// kernels against them. The product library (FLEXPAI_XCHECK 0) does not contain them and ignores those variables.
#ifndef FLEXPAI_XCHECK
#define FLEXPAI_XCHECK 0
#endif
static const char* xcheck_env(const char* name) {
#if FLEXPAI_XCHECK
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}
#include "engine_pair.hpp"
#include "engine_dec4.hpp"
#include "engine_grp_pair.hpp"
#include "engine_pe.hpp"
#include "engine_pfb.hpp"
#include "engine_sgp.hpp"
#include "engine_sgs.hpp"
#include "engine_grp.hpp"
#include "engine_mul.hpp"
#include "engine_mm.hpp"
#include "engine_sd.hpp"
#include "engine_hist.hpp"
#include "engine_shist.hpp"
#include "engine_scan.hpp"
#include "engine_obf.hpp"
#include "engine_pack.hpp"
#include "engine_foldw.hpp"
#include "engine_res.hpp"
#include "engine_pool.hpp"
#include "engine_crtw.hpp"
#include "engine_pe1.hpp"
#include "engine_pe4.hpp"
#include "engine_crt4.hpp"
#include "encrypt_route.hpp"

using namespace fpai;

static thread_local std::string g_last_error;

static int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
#define HIPCHK(expr)                                                                    \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) return fail(PAI_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)

// Largest call (elements) whose CRT exponentiations run on 16-lane rows (k_crt_w) instead of lanes / lane pairs
// (k_crt_a + k_crt_b_pair): below it the lane kernels leave the chip mostly idle and take one lane's whole chain.
// The test build keeps 0, so that its contexts -- the cross-checks' references -- stay on the kernels the rows stand in for.
constexpr long long CRTW_DEFAULT_MAX = FLEXPAI_XCHECK ? 0 : 4096;

// Device allocations that are released together: plain hipMalloc blocks (constants) and TableArena blocks (tables)
static void free_device(std::vector<void*>& mem, std::vector<void*>& tables) {
  for (void* p : mem) (void)hipFree(p);
  for (void* p : tables) TableArena::get().free(p);
  mem.clear();
  tables.clear();
}

// Everything one build of the key holder's fixed-base tables produced (ensure_fb). release() frees the memory and
// returns every field to its default, so nothing of a released build can be read again.
struct FbTables {
  int K = 0;                    // digit positions
  int W_used = 0;               // window of the resident tables (may be below pai_ctx::fb_W under a memory cap)
  int nw = 0;                   // Shoup rows: positions 0 .. nw-1 are one bit wider than the window (fb_cut.hpp)
  int raw_bits = 0;
  FbRed* d_red = nullptr;       // [2] k_fb_digits: the exponent reduction mod p_h - 1
  // 1024/2048-bit keys: pair tables over the S limbs of p_h
  int pair_s = 0;               // S (19 / 37); 0 = no pair tables
  bool shoup = false;           // Shoup rows (kernels_fbs.hpp, k_fbs); the test build's $FLEXPAI_FBS=0: Montgomery rows (k_fbp)
  FbpHalf* d_fbp = nullptr;     // [2]
  FbsConst* d_fbs_cst = nullptr;   // [2] k_fbs_fill's constants (table construction only)
  uint32_t* d_fbp_fin_cs = nullptr;        // k_fbp_fin: its 12 S constant words,
  const uint32_t* d_fbp_fin_p = nullptr;   //   p
  uint32_t fbp_fin_mprime = 0;
  // 4096-bit keys: pair-group tables (kernels_grp_pair.hpp)
  bool gpair = false;
  FbgpHalf* d_fbgp = nullptr;   // [2]
  SgpHalf* d_sgp = nullptr;     // [2] the split-pair sampler over the same tables (kernels_sgp.hpp)
  SgsHalf* d_sgs = nullptr;     // [2]   ... on Shoup rows (kernels_sgs.hpp)
  const uint32_t* d_sgp_q = nullptr;   // q's S limbs (k_sgp_fin)
  const uint32_t* d_m0 = nullptr;                 // k_fbg_garner: p^2 (FbgpHalf::p2 of the p half),
  uint32_t *d_m8 = nullptr, *d_coefR = nullptr;   //   8 p^2, (q^2)^-1 R mod p^2
  uint32_t mprime0 = 0;         //   ... and p^2's Montgomery constant
  uint32_t* d_q2Rn = nullptr;   // q^2 R mod n^2 (k_fbg_fin)
  std::vector<void*> mem;       // the constants above
  std::vector<void*> tables;    // the tables themselves (TableArena: pooled device memory)
  float host_ms = 0.f, dev_ms = 0.f;
  uint64_t table_bytes = 0;
  void release() {
    free_device(mem, tables);
    *this = FbTables();
  }
};

// The same for the public-key tables (ensure_pfb)
struct PfbTables {
  int K = 0, K0 = 0, W_used = 0;   // digit positions (K0 of them e_0's), window
  PfbConst* d_pfb = nullptr;
  SgpHalf* d_sgp = nullptr;        // the split-pair sampler over the public tables (kernels_sgp.hpp)
  std::vector<void*> mem, tables;
  void release() {
    free_device(mem, tables);
    *this = PfbTables();
  }
};

struct pai_ctx {
  int device = 0;
  int nb = 0;
  int tpi_e = 0, S_e = 0;
  int tpi_d = 0, S_d = 0;
  int ct_words = 0, pt_words = 0;
  HBig n, N;
  uint32_t mprime_N = 0;
  uint32_t *d_N = nullptr, *d_R2 = nullptr, *d_nl = nullptr;
  uint32_t* d_pew_prog = nullptr;   // op list over n for k_pe_w (public-key encryption on 16-lane rows)
  int pew_nprog = 0;
  uint32_t* d_prog = nullptr;   // Montgomery program for x^n (run_program, kernels.hpp)
  int nprog = 0;
  uint32_t* d_oneR = nullptr;   // R mod n^2
  uint32_t* d_RS = nullptr;     // [ADD_KMAX + 2][ct_words]: R^s mod n^2 (k_add's Montgomery corrections)
  void* d_addplan = nullptr;    // k_add schedule sort: buckets, permutation, histogram
  size_t addplan_bytes = 0;
  // private key material
  bool has_priv = false;
  DecHalf* d_halves = nullptr;
  uint32_t *d_qinvR = nullptr, *d_nlimb = nullptr, *d_qRn = nullptr, *d_maxint = nullptr;
  uint32_t nprime_d = 0;
  int nwin = 0, n_limbs = 0;
  // CRT encryption (kernels_crt.hpp): available when the private key is set and the halves fit
  bool crt_ok = false;
  bool fbg_ok = false;        // 4096-bit keys: fixed-base sampler on the group engine (engine_grp), no lane CRT
  bool crt_enabled = true;
  // calls of up to crtw_max elements run the CRT exponentiations on 16-lane rows (kernels_crtw.hpp: latency of
  // protocol-sized calls); PAI_OPT_ROWS_MAX
  long long crtw_max = CRTW_DEFAULT_MAX;
  int crt_sa = 0, crt_sb = 0;
  int rows_sa = 0;   // 74: a 4096-bit key's row-kernel constants (k_crt_w<74, 148>, k_dec_w<74, 148>; setup_rows4096)
  CrtHalf* d_crt_a = nullptr;   // [2] stage A halves
  CrtHalf* d_crt_b = nullptr;   // [2] stage B halves
  uint32_t *d_kq = nullptr, *d_kp = nullptr;
  // lane-engine CRT decryption (kernels_dec.hpp): same sizes as the CRT encryption halves
  bool dec_lane_ok = false;
  bool dec_lane_enabled = true;
  // p-adic pair exponentiations (kernels_pair.hpp): decryption and CRT stage B on the S limbs of p_h;
  // the default for 1024/2048-bit keys ($FLEXPAI_PAIR=0 selects the 2S-limb lane kernels)
  bool dec_pair_ok = false, crt_pair_ok = false;
  DecPairHalf* d_decp_halves = nullptr;
  CrtHalf* d_decp_pow = nullptr;   // decryption halves; c0: the factored chain's K'_t ([16][S], decf)
  bool decf = false;                // the factored (B-free) decryption chain (kernels_pair.hpp decf_run)
  CrtHalf* d_crtp_b = nullptr;
  CrtHalf* d_decw = nullptr;   // [2] k_dec_w's halves (kernels_crtw.hpp): p_h^2, R^(K+1), 1, op list over p_h - 1
  int decw_kchunks = 0;
  uint32_t *d_decp_nl = nullptr, *d_decp_maxint = nullptr;
  int decp_kchunks = 0;
  // 4096-bit keys: decryption on split pairs (kernels_dec4.hpp), the default; the group k_decrypt otherwise
  bool dec4_ok = false;
  Dec4Half* d_dec4_halves = nullptr;
  int dec4_kchunks = 0;
  // 2049..4096-bit keys: the key holder's CRT encryption above the rows on split pairs (kernels_crt4.hpp; stage A reads
  // setup_rows4096's d_crt_a). Calls of at most crt4_min elements stay on k_encrypt<8> (PAI_OPT_CRT4_MIN)
  bool crt4_ok = false;
  Crt4Half* d_crt4_b = nullptr;
  long long crt4_min = 128;
  // public-key encryption on split pairs (kernels_pe.hpp): 2048-bit n, the default ($FLEXPAI_PAIR=0: k_encrypt)
  bool pe_ok = false;
  // public-key encryption of n <= 1024 bits on pairs over the 37 limbs of n (kernels_pe1.hpp)
  bool pe1_ok = false;
  DecPairHalf* d_pe1_half = nullptr;   // n, the pair of R^3 mod n^2 (k_dec_pre_pair's constants)
  uint32_t *d_pe1_n = nullptr, *d_pe1_one = nullptr, *d_pe1_prog = nullptr, *d_pe1_r2n = nullptr;
  int pe1_nprog = 0;
  uint32_t pe1_mprime = 0;
  // public-key encryption of n of 2049..4096 bits on pair groups over the 152 limbs of n (kernels_pe4.hpp); taken by
  // contexts without the private key ($FLEXPAI_PAIR=0, test build: k_encrypt)
  bool pe4_ok = false;
  Pe4Const* d_pe4 = nullptr;
  bool pef_ok = false;          // the factored public-key chain (k_pe_pow_f) is set up ($FLEXPAI_PEF=0, test build: off)
  PeConst* d_pe = nullptr;
  uint32_t *d_pe_n = nullptr, *d_pe_r2 = nullptr, *d_pe_oneR = nullptr;   // n, R^2, R mod n (R = 2^(28 74)): the batch
  uint32_t pe_mprime = 0;                                                 //   inversion of the bases mod n (TPI = 2)
  uint32_t *d_dec_p = nullptr, *d_dec_q = nullptr, *d_dec_qinvR = nullptr;   // (k_dec_fin_pair's CRT constants)
  uint32_t dec_pprime = 0;
  // fixed-base obfuscation (kernels_fb.hpp): device-RNG encryption for key holders. Built lazily on
  // the first PAI_OBF_RNG encryption (or pai_ctx_fixed_base_prepare); any failure (key shape, table
  // memory) leaves the generic CRT path in charge and never affects decryption.
  enum { FB_UNTRIED = 0, FB_READY = 1, FB_UNAVAILABLE = 2 };
  int fb_state = FB_UNTRIED;
  std::string fb_reason;        // why the fixed-base path is unavailable
  bool fb_enabled = true;
  int fb_W = 0;                 // requested digit window (bits); 0 = not chosen yet ($FLEXPAI_FB_WINDOW, default 16)
  uint32_t fb_g[2] = {0, 0};   // the bases g_p, g_q (generators of Z_p*, Z_q*)
  HBig fb_p, fb_q;              // p < q
  FbTables fb;                  // the resident tables and their constants (rebuilt when the window changes)
  uint32_t* fb_last_w = nullptr;  // debugging: the sampler's output of the last chunk (pai_debug_fb_w), in d_work
  long long fb_last_n = 0;
  GuardRec* d_guard = nullptr;  // test build: the address guards' record (guard.hpp); null in the product
  // public-key fixed-base obfuscators (kernels_pfb.hpp): device-RNG encryption without the private key.
  // Built lazily past the break-even count (or pai_ctx_public_fb_prepare); never needed for correctness.
  int pfb_state = FB_UNTRIED;
  std::string pfb_reason;
  bool pfb_enabled = true;
  int pfb_W = 0;                // requested window; 0 = not chosen yet
  std::vector<HBig> pfb_bases;  // g_0 .. g_PFB_SHORT (chosen at the first build unless set)
  PfbTables pfb;
  long long pfb_seen = 0;
  long long fb_seen = 0;        // device-RNG elements encrypted under this key before the tables exist
  int fb_call = 0;              // host-buffer call in progress: its one fixed-base decision (+1 / -1), else 0
  int pfb_call = 0;             // the same for the public fixed-base sampler
  bool stage_keep = false;      // host-buffer calls: stage timing spans all chunks of the call
  std::vector<void*> allocs;
  std::vector<void*> priv_allocs;   // private-key constants: all freed together if set_private fails
  bool in_priv = false;             // upload() targets priv_allocs
  // scratch (exponent tables), grown on demand
  void* d_scratch = nullptr;
  size_t scratch_bytes = 0;
  void* d_work = nullptr;       // CRT intermediates (y, u)
  size_t work_bytes = 0;
  void* d_mul = nullptr;        // ciphertext x plaintext terms, flags, reduction partials
  size_t mul_bytes = 0;
  void* d_seg = nullptr;        // segmented sums: gather rows and the partial sums of each level
  size_t seg_bytes = 0;
  void* d_take = nullptr;       // pai_take_dev's row index; pai_check_below_dev's result word
  size_t take_bytes = 0;
  uint32_t* d_nsq32 = nullptr;  // n^2 in 32-bit words (pai_check_below_dev), uploaded at its first call
  void* d_plain = nullptr;      // ciphertext + plaintext: the two k_add operands and their exponents
  size_t plain_bytes = 0;
  // re-randomisation (pai_obfuscate_dev): the zero plaintexts, scratch exponents and statuses of the encryption that
  // yields r^n, and, for in-place calls, r^n of one slice of obf_chunk elements (PAI_OPT_OBF_CHUNK)
  void* d_obf = nullptr;
  size_t obf_bytes = 0;
  int obf_chunk = 262144;
  // packed plaintexts (kernels_pack.hpp): the zero plaintexts, exponents and statuses of the encryption that yields r^n
  // (pai_encrypt_packed_dev); the exponents, values, statuses and raw plaintexts of the decrypt chain ahead of k_unpack
  // (pai_decrypt_packed_dev); and k_unpack's constants, the words of n, max_int and n - max_int
  void* d_pack = nullptr;
  size_t pack_bytes = 0;
  uint32_t* d_pack_consts = nullptr;
  // obfuscator pool (kernels_pool.hpp): a FIFO ring of ready r^n in split rows, the constants of its kernels (they depend
  // on n alone and are uploaded with the first ring), and the plain rho of the composed path (PAI_OPT_POOL_FUSED = 0)
  struct Pool {
    uint32_t* rows = nullptr;     // [cap][row_words], dev_malloc
    size_t cap = 0, head = 0, ready = 0;
    uint64_t taken = 0;           // entries consumed over the context's life
    int row_words = 0;
    uint32_t *d_nneg = nullptr, *d_R2n = nullptr, *d_R2n84 = nullptr;
    uint32_t nprime = 0, dprime = 0;
    bool consts = false;
    bool fused = true;            // PAI_OPT_POOL_FUSED
    void* d_rho = nullptr;
    size_t rho_bytes = 0;
  } pool;
  // fused matrix product (kernels_mm.hpp): PAI_OPT_MATMUL_FUSED / PAI_OPT_MATMUL_PATH
  bool mm_fused = true;
  int mm_path = 0;              // last pai_matmul[_dev] call: 0 none yet, 1 term path, 2 fused
  void* d_mmtab = nullptr;      // window tables of one block of ciphertexts (at most the table budget)
  size_t mmtab_bytes = 0;
  void* d_mmwork = nullptr;     // neg_row [K], the inversion's flags [m K]
  size_t mmwork_bytes = 0;
  void* d_mminv = nullptr;      // copy of the ciphertexts with the flagged rows' inverted (only with negative scalars)
  size_t mminv_bytes = 0;
  std::vector<uint8_t> mm_neg, mm_flags;   // host sides of neg_row and of the flags
  // segmented weighted sums (kernels_sd.hpp): PAI_OPT_SEGDOT_FUSED / PAI_OPT_SEGDOT_PATH
  bool sd_fused = true;
  int sd_path = 0;              // last pai_segment_dot[_dev] call: 0 none yet, 1 term path, 2 fused
  void* d_sdmeta = nullptr;     // index, chunk starts, table slots, block rows, sign flags
  size_t sdmeta_bytes = 0;
  void* d_sdbuf = nullptr;      // a slice's gathered entries and terms (term path) / a block's distinct ciphertexts (fused)
  size_t sdbuf_bytes = 0;
  void* d_sdpart = nullptr;     // the chunk partials and their exponents
  size_t sdpart_bytes = 0;
  // host sides of the metadata (they outlive the call's asynchronous copies)
  struct SdHost {
    std::vector<long long> cstart, segch, iota, urows, rows;
    std::vector<int32_t> uid, tslot, idmap;
    std::vector<uint8_t> neg, flags;
  } sd;
  // histograms (kernels_hist.hpp): the scratch budget of one feature block, the device buffers and the host sides
  // of the metadata (they outlive the call's asynchronous copies)
  size_t hist_scratch = (size_t)256 << 20;
  void* d_histmeta = nullptr;   // counts (when the caller wants none), member offsets, cursors, runs
  size_t histmeta_bytes = 0;
  void* d_histwork = nullptr;   // one feature block's member lists and gather rows
  size_t histwork_bytes = 0;
  void* d_histpart = nullptr;   // the runs' partials and their exponents
  size_t histpart_bytes = 0;
  struct HistHost {
    std::vector<long long> cnt, index, segoff;
    std::vector<int32_t> cell_off;
    std::vector<int2> runs;
    // pai_histogram_sparse (kernels_shist.hpp): read-backs of the checks, the default bins, and the default step's lists
    long long nnz = 0;
    unsigned err = 0;
    std::vector<int32_t> zs, smem;
    std::vector<int2> sruns;
    std::vector<long long> sgidx, scount;
  } hist;
  void* d_shist = nullptr;      // sparse histograms: the slot sums, the S values after them, and their exponents
  size_t shist_bytes = 0;
  void* d_shisterr = nullptr;   // the error bits of the CSR checks
  size_t shisterr_bytes = 0;
  // prefix sums (kernels_scan.hpp): PAI_OPT_SCAN_TILE / PAI_OPT_SCAN_PATH
  int scan_tile = 0;            // 0: automatic tile length of the blocked path
  int scan_path = 0;            // last pai_cumsum[_dev] call: 0 none yet, 1 row chains, 2 blocked
  // folds (kernels_pack.hpp k_pack_fold, kernels_foldw.hpp k_pack_fold_w): PAI_OPT_FOLD_ROWS / PAI_OPT_FOLD_PATH
  int fold_rows = 1;            // 1 automatic (fold_rows_max), 0 never rows, 2 rows wherever a row kernel exists
  int fold_path = 0;            // last pai_pack_ciphertexts[_dev] / pai_repack[_dev] call: 0 none yet, 1 groups, 2 rows
  long long fold_call_n = 0;    // outputs of the host-buffer fold in progress (its chunks share one choice), else 0
  void* d_scan = nullptr;       // the blocked path's tile totals and their scans, all levels
  size_t scan_bytes = 0;
  void* d_inv = nullptr;        // batch-inversion prefix products and segment products
  size_t inv_bytes = 0;
  std::vector<uint32_t> inv_host;   // top of the inversion tree (host side of an async copy)
  // the public-key chain's inversion without a host wait (batch_invert_async): the top value goes device -> pinned
  // words, a host function in stream order inverts it mod n there, and the result (+ a no-inverse flag) goes back
  struct AsyncInv {
    HBig mod;
    int W = 0;
    uint32_t* pin = nullptr;     // [W] words of the top value, then its inverse; [W]: 1 = no inverse exists
  };
  AsyncInv* inv_async = nullptr;
  int cus = 0;
  // optional per-stage timing of the last encrypt call (PAI_OPT_STAGE_TIMING)
  bool timing = false;
  // HIP events between the kernels of each chunk of the last encrypt / decrypt call; the stage times
  // are summed over its chunks (a call of more than CRT_CHUNK elements runs several)
  std::vector<std::array<hipEvent_t, 4>> ev;   // per chunk of the timed call; grown on demand, read at the query
  int nev = 0, nchunk_ev = 0;
  // host-buffer entry points (pai_encrypt / pai_decrypt / pai_add): device copies of the operands, a
  // compute and a copy stream, one event per chunk (host_pipe below)
  void* d_hostio = nullptr;
  size_t hostio_bytes = 0;
  hipStream_t s_comp = nullptr, s_copy = nullptr;
  std::vector<hipEvent_t> hev, pev;   // per chunk: kernels done / staging copy done
  std::vector<hipEvent_t> oev;        // pai_obfuscate, whose hev mark the uploads: per chunk, kernels done
  void* h_pin[2] = {nullptr, nullptr};  // pinned staging slots (PCIe at full rate, truly asynchronous)
  size_t pin_bytes = 0;
  // thread safety (CtxLock below): one call at a time per context, and the device work of successive calls
  // ordered through tail_ev even when they come on different streams
  mutable std::recursive_mutex mu;
  hipEvent_t tail_ev = nullptr;
  bool counted = false, holder = false;   // in g_contexts / g_key_holders
  ~pai_ctx();
};

static std::atomic<int> g_contexts{0}, g_key_holders{0};

// $FLEXPAI_SETUP_TRACE=1: wall time of each per-key setup step on stderr ("flexpai-trace <step> <ms>"), and the count
// and time of the constant uploads (the fresh-key analysis of DESIGN §5; tools/fresh_key_trace.py)
static bool setup_trace_on() {
  static const bool on = getenv("FLEXPAI_SETUP_TRACE") != nullptr;
  return on;
}
static std::atomic<long> g_upload_n{0};
static std::atomic<long long> g_upload_ns{0};
struct SetupTrace {
  const char* name;
  std::chrono::steady_clock::time_point t0;
  explicit SetupTrace(const char* n) : name(n), t0(std::chrono::steady_clock::now()) {}
  ~SetupTrace() {
    if (setup_trace_on())
      fprintf(stderr, "flexpai-trace %-32s %10.3f ms\n", name,
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
};
static void trace_uploads(const char* where) {
  if (!setup_trace_on()) return;
  fprintf(stderr, "flexpai-trace %-32s %10.3f ms (%ld uploads)\n", where, (double)g_upload_ns.exchange(0) * 1e-6,
          g_upload_n.exchange(0));
}

pai_ctx::~pai_ctx() {
  if (counted) --g_contexts;
  if (holder) --g_key_holders;
  (void)hipSetDevice(device);
  if (tail_ev) {
    (void)hipEventSynchronize(tail_ev);
    (void)hipEventDestroy(tail_ev);
  }
  for (auto& ch : ev)
    for (auto& e : ch)
      if (e) (void)hipEventDestroy(e);
  for (auto& e : hev) (void)hipEventDestroy(e);
  for (auto& e : pev) (void)hipEventDestroy(e);
  for (auto& e : oev) (void)hipEventDestroy(e);
  for (void* p : h_pin)
    if (p) (void)hipHostFree(p);
  if (s_comp) (void)hipStreamDestroy(s_comp);
  if (s_copy) (void)hipStreamDestroy(s_copy);
  if (d_hostio) (void)hipFree(d_hostio);
  if (d_guard) (void)hipFree(d_guard);
  for (void* p : allocs) (void)hipFree(p);
  for (void* p : priv_allocs) (void)hipFree(p);
  fb.release();
  pfb.release();
  if (counted && g_contexts.load() == 0) TableArena::get().trim();   // the process's last context: pooled chunks go back
  if (d_scratch) (void)hipFree(d_scratch);
  if (d_work) (void)hipFree(d_work);
  if (d_mul) (void)hipFree(d_mul);
  if (d_mmtab) (void)hipFree(d_mmtab);
  if (d_mmwork) (void)hipFree(d_mmwork);
  if (d_mminv) (void)hipFree(d_mminv);
  if (d_sdmeta) (void)hipFree(d_sdmeta);
  if (d_sdbuf) (void)hipFree(d_sdbuf);
  if (d_sdpart) (void)hipFree(d_sdpart);
  if (d_histmeta) (void)hipFree(d_histmeta);
  if (d_histwork) (void)hipFree(d_histwork);
  if (d_histpart) (void)hipFree(d_histpart);
  if (d_shist) (void)hipFree(d_shist);
  if (d_shisterr) (void)hipFree(d_shisterr);
  if (d_scan) (void)hipFree(d_scan);
  if (d_inv) (void)hipFree(d_inv);
  if (inv_async) {
    if (inv_async->pin) (void)hipHostFree(inv_async->pin);
    delete inv_async;
  }
  if (d_plain) (void)hipFree(d_plain);
  if (d_obf) (void)hipFree(d_obf);
  if (d_pack) (void)hipFree(d_pack);
  if (pool.rows) (void)hipFree(pool.rows);
  if (pool.d_rho) (void)hipFree(pool.d_rho);
  if (d_seg) (void)hipFree(d_seg);
  if (d_take) (void)hipFree(d_take);
  if (d_addplan) (void)hipFree(d_addplan);
}

// Held by every entry point that takes a context, for the whole call (recursive: the host-buffer entry points
// call the *_dev ones). A context's device buffers -- scratch, work, fixed-base tables, host-io carve-outs --
// are shared by all its calls, so a *_dev call's stream first waits for the device work of the context's
// previous call (whatever stream that was on) and the call's own work becomes the new tail. Two threads may
// therefore share one context: their calls run one after the other, on the host and on the device (SURVEY.md
// §8(b)(iv); the reference isolates its state per process instead, encryptor.py:89-96).
struct CtxLock {
  pai_ctx* c;
  hipStream_t st = nullptr;
  bool dev = false;
  std::unique_lock<std::recursive_mutex> lk;
  explicit CtxLock(const pai_ctx* ctx) : c(const_cast<pai_ctx*>(ctx)), lk(ctx->mu) {}
  CtxLock(pai_ctx* ctx, hipStream_t s) : c(ctx), st(s), dev(true), lk(ctx->mu) {
    (void)hipSetDevice(c->device);
    if (c->tail_ev) (void)hipStreamWaitEvent(st, c->tail_ev, 0);
  }
  ~CtxLock() {
    if (!dev) return;
    if (!c->tail_ev && hipEventCreateWithFlags(&c->tail_ev, hipEventDisableTiming) != hipSuccess) {
      c->tail_ev = nullptr;
      (void)hipGetLastError();
      return;
    }
    (void)hipEventRecord(c->tail_ev, st);
  }
};

// v -> a device block of its own, owned by `owner` (whoever holds that list frees it)
template <typename T>
static int upload_to(std::vector<void*>& owner, const std::vector<T>& v, T** out) {
  const auto t0 = std::chrono::steady_clock::now();
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, std::max<size_t>(v.size(), 1) * sizeof(T)));
  owner.push_back(p);
  if (!v.empty()) HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *out = (T*)p;
  ++g_upload_n;
  g_upload_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}
template <typename T>
static int upload(pai_ctx* c, const std::vector<T>& v, T** out) {
  return upload_to(c->in_priv ? c->priv_allocs : c->allocs, v, out);
}

static void append(std::vector<uint32_t>& to, const std::vector<uint32_t>& v) { to.insert(to.end(), v.begin(), v.end()); }

// v < P^2 as the pair [v mod P : limbs][v div P : limbs] of 28-bit limbs (the pair kernels' residues mod P^2)
static std::vector<uint32_t> pair_split(const HBig& v, const HBig& P, int limbs) {
  const HBig qt = div_big(v, P);
  std::vector<uint32_t> out = sub(v, mul(qt, P)).limbs(limbs, LB);
  append(out, qt.limbs(limbs, LB));
  return out;
}

static int tpi_for_bits(size_t need_bits, int min_tpi) {
  for (int t : {1, 2, 4, 8})
    if (t >= min_tpi && (size_t)LB * L * t >= need_bits) return t;
  return 0;
}

// left-to-right sliding window (k = 5) over the fixed public exponent n
static void sliding_schedule(const HBig& e, std::vector<uint16_t>& ops, int& first) {
  const int K = 5;
  int i = (int)e.bits() - 1;
  auto window = [&](int hi, int& lo, uint32_t& val) {
    lo = std::max(hi - K + 1, 0);
    while (!e.bit(lo)) ++lo;
    val = 0;
    for (int b = hi; b >= lo; --b) val = (val << 1) | (uint32_t)e.bit(b);
  };
  int lo;
  uint32_t v;
  window(i, lo, v);
  first = (int)(v - 1) / 2;
  i = lo - 1;
  int nsq = 0;
  while (i >= 0) {
    if (!e.bit(i)) {
      ++nsq;
      --i;
      continue;
    }
    window(i, lo, v);
    nsq += i - lo + 1;
    ops.push_back((uint16_t)nsq);
    ops.push_back((uint16_t)((v - 1) / 2));
    nsq = 0;
    i = lo - 1;
  }
  if (nsq) {
    ops.push_back((uint16_t)nsq);
    ops.push_back(0xFFFF);
  }
}

// Op list for run_program: x~ = x R (the caller puts R^2 in the slot), odd powers x~^(2k+1) into
// tiles k = 0..15, then the left-to-right sliding-window chain over e. The kernel appends the final
// product with tile T_FINAL.
static bool build_modexp_program(const HBig& e, std::vector<uint32_t>& prog) {
  std::vector<uint16_t> sched;
  int first = 0;
  sliding_schedule(e, sched, first);
  auto op = [](uint32_t flags, int bidx, int aidx, int sidx) {
    return flags | ((uint32_t)bidx << 8) | ((uint32_t)aidx << 16) | ((uint32_t)sidx << 24);
  };
  prog.clear();
  prog.push_back(op(OP_STORE, 0, 0, 0));                                  // x~ = x R        -> T0
  prog.push_back(op(OP_B_FROM_A, 0, 0, 0));                               // x~^2
  prog.push_back(op(OP_B_FROM_A | OP_A_FROM_T | OP_STORE, 0, 0, 1));      // x~^3           -> T1
  for (int k = 2; k < TABLE_ODD; ++k) prog.push_back(op(OP_STORE, 0, 0, k));   // x~^(2k+1) -> Tk
  bool loaded = false;   // accumulator still to be taken from tile `first`
  for (size_t i = 0; i + 1 < sched.size(); i += 2) {
    const int nsq = sched[i], idx = sched[i + 1];
    for (int t = 0; t < nsq; ++t) {
      prog.push_back(loaded ? op(OP_B_FROM_A, 0, 0, 0) : op(OP_B_FROM_T | OP_A_FROM_T, first, first, 0));
      loaded = true;
    }
    if (idx != 0xFFFF) {
      prog.push_back(loaded ? op(OP_B_FROM_A | OP_A_FROM_T, 0, idx, 0) : op(OP_B_FROM_T | OP_A_FROM_T, first, idx, 0));
      loaded = true;
    }
  }
  return loaded;   // false only for single-window exponents, which n (odd, >= 64 bits) never is
}

// Op list for run_lane_program (kernels_crt.hpp): the kernel stores x~ in tile 0; odd powers into
// tiles 0..15 (x~^2 kept as the LDS multiplier), then the sliding-window chain over e.
static bool build_lane_program(const HBig& e, std::vector<uint32_t>& prog) {
  if (e.bits() < 8) return false;
  std::vector<uint16_t> sched;
  int first = 0;
  sliding_schedule(e, sched, first);
  auto op = [](uint32_t flags, int bidx, int aidx, int sidx) {
    return flags | ((uint32_t)bidx << 8) | ((uint32_t)aidx << 16) | ((uint32_t)sidx << 24);
  };
  prog.clear();
  prog.push_back(op(LOP_SQR | LOP_B_SET, 0, 0, 0));                       // x~^2 -> LDS multiplier
  prog.push_back(op(LOP_A_FROM_T | LOP_B_READY | LOP_STORE, 0, 0, 1));    // x~ * x~^2  -> T1
  for (int k = 2; k < 16; ++k) prog.push_back(op(LOP_STORE | LOP_B_READY, 0, 0, k));   // multiplier x~^2 kept
  bool loaded = false;
  size_t first_sq = SIZE_MAX;   // first squaring since the last multiply (prefetch slot)
  for (size_t i = 0; i + 1 < sched.size(); i += 2) {
    const int nsq = sched[i], idx = sched[i + 1];
    for (int t = 0; t < nsq; ++t) {
      if (first_sq == SIZE_MAX) first_sq = prog.size();
      prog.push_back(loaded ? op(LOP_SQR, 0, 0, 0) : op(LOP_SQR | LOP_A_FROM_T, 0, first, 0));
      loaded = true;
    }
    if (idx != 0xFFFF) {
      if (first_sq != SIZE_MAX) {
        prog[first_sq] |= LOP_PREFETCH | ((uint32_t)idx << 8);
        prog.push_back(op(LOP_B_READY, idx, 0, 0));
      } else {
        prog.push_back(loaded ? op(0, idx, 0, 0) : op(LOP_A_FROM_T, idx, first, 0));
      }
      loaded = true;
      first_sq = SIZE_MAX;
    }
  }
  return loaded;
}

// Stage A's exponent, other mod (p_h - 1). Primes that lie close to one another, or to powers of two in the ratio
// 2^k (the two largest primes below 2^517; 2^518 - 917 and 2^517 - 489, which leave 63), give a residue too short for
// an op list (build_lane_program wants a chain of more than one window). Such a residue is lifted by p_h - 1, which
// changes no result: x^(p_h - 1) = 1 mod p_h for every unit, and a multiple of p_h stays 0 (it would not at residue 0).
static HBig stage_a_exponent(const HBig& other, const HBig& ph) {
  const HBig pm1 = sub(ph, HBig(1));
  const HBig ea = mod(other, pm1);
  return ea.bits() < 64 ? add(ea, pm1) : ea;
}

// K_t: for each table entry t, the sum over the chain's multiplies by it of 2^(squares after that multiply)
static std::vector<HBig> chain_weights(const HBig& ph, const std::vector<uint16_t>& sched) {
  std::vector<HBig> K(LANE_NTILE, HBig(0));
  size_t after = 0;
  for (size_t i = sched.size(); i >= 2; i -= 2) {
    const int nsq = sched[i - 2], idx = sched[i - 1];
    if (idx != 0xFFFF) K[idx] = mod(add(K[idx], mul_pow2_mod(HBig(1), after, ph)), ph);
    after += (size_t)nsq;
  }
  return K;
}

// Op list of the factored 1024/2048-bit decryption (decf_run, kernels_pair.hpp; tools/decf_model.py): the table of
// full pairs as build_lane_program (x~^2 general, kept in the column; odd powers into tiles 0..15), the chain over
// e = p_h - 2 with B-free multipliers (LOP_BFREE), then Y' (A~, 0) (iota put into the column before it) and the
// product with (1, 0). kf: the closing Horner sum's K'_t = R (K_t + [t == 0]) mod p_h, S limbs each (entry 1's
// weight + 1: the closing (A~, 0) drops its (1 + p b_1)).
static bool build_decf_lane_program(const HBig& ph, size_t RS, int S, std::vector<uint32_t>& prog, std::vector<uint32_t>& kf) {
  const HBig e = sub(ph, HBig(2));
  if (e.bits() < 8) return false;
  std::vector<uint16_t> sched;
  int first = 0;
  sliding_schedule(e, sched, first);
  auto op = [](uint32_t flags, int bidx, int aidx, int sidx) {
    return flags | ((uint32_t)bidx << 8) | ((uint32_t)aidx << 16) | ((uint32_t)sidx << 24);
  };
  prog.clear();
  prog.push_back(op(LOP_SQR | LOP_B_SET, 0, 0, 0));                       // x~^2 -> LDS multiplier
  prog.push_back(op(LOP_A_FROM_T | LOP_B_READY | LOP_STORE, 0, 0, 1));    // x~ * x~^2  -> T1
  for (int k = 2; k < LANE_NTILE; ++k) prog.push_back(op(LOP_STORE | LOP_B_READY, 0, 0, k));
  bool loaded = false;
  size_t first_sq = SIZE_MAX;
  for (size_t i = 0; i + 1 < sched.size(); i += 2) {
    const int nsq = sched[i], idx = sched[i + 1];
    for (int t = 0; t < nsq; ++t) {
      if (first_sq == SIZE_MAX) first_sq = prog.size();
      prog.push_back(loaded ? op(LOP_SQR, 0, 0, 0) : op(LOP_SQR | LOP_A_FROM_T, 0, first, 0));
      loaded = true;
    }
    if (idx != 0xFFFF) {
      if (first_sq != SIZE_MAX) {
        prog[first_sq] |= LOP_PREFETCH | ((uint32_t)idx << 8);
        prog.push_back(op(LOP_B_READY | LOP_BFREE, idx, 0, 0));
      } else {
        prog.push_back(loaded ? op(LOP_BFREE, idx, 0, 0) : op(LOP_A_FROM_T | LOP_BFREE, idx, first, 0));
      }
      loaded = true;
      first_sq = SIZE_MAX;
    }
  }
  if (!loaded) return false;
  prog.push_back(op(LOP_IOTA | LOP_BFREE, 0, 0, 0));      // Z = Y' (A~, 0), iota = Y' mod p -> the column
  prog.push_back(op(LOP_B_CONST | LOP_BFREE, 0, 0, 0));   // (1 + p G) = Z (1, 0)
  std::vector<HBig> K = chain_weights(ph, sched);
  K[0] = mod(add(K[0], HBig(1)), ph);
  kf.clear();
  for (int t = 0; t < LANE_NTILE; ++t) {
    const std::vector<uint32_t> l = mul_pow2_mod(K[t], RS, ph).limbs(S, LB);
    kf.insert(kf.end(), l.begin(), l.end());
  }
  return true;
}

// Op list of the factored public-key chain (d4f_run<S, true>, kernels_pe.hpp k_pe_pow_f): the table's 30 one-pass
// products by the kept (A_r, 0) (odd powers into tiles 0..15, tile 0 = (A_r, 0)), the sliding-window chain over n with
// B-free multipliers, then the product with (1, 0) into tile D4F_G. kf: K'_t = R K_t mod n (entry 1 is B-free: H_1 = 0).
static bool build_pef_program(const HBig& n, size_t RS, std::vector<uint32_t>& prog, std::vector<uint32_t>& kf) {
  if (n.bits() < 8) return false;
  std::vector<uint16_t> sched;
  int first = 0;
  sliding_schedule(n, sched, first);
  auto op = [](uint32_t flags, int bidx, int aidx, int sidx) {
    return flags | ((uint32_t)bidx << 8) | ((uint32_t)aidx << 16) | ((uint32_t)sidx << 24);
  };
  prog.clear();
  for (int t = 2; t < 2 * LANE_NTILE; ++t) prog.push_back(op(LOP_B_READY | ((t & 1) ? LOP_STORE : 0u), 0, 0, (t - 1) / 2));
  bool loaded = false;
  size_t first_sq = SIZE_MAX;
  for (size_t i = 0; i + 1 < sched.size(); i += 2) {
    const int nsq = sched[i], idx = sched[i + 1];
    for (int t = 0; t < nsq; ++t) {
      if (first_sq == SIZE_MAX) first_sq = prog.size();
      prog.push_back(loaded ? op(LOP_SQR, 0, 0, 0) : op(LOP_SQR | LOP_A_FROM_T, 0, first, 0));
      loaded = true;
    }
    if (idx != 0xFFFF) {
      if (first_sq != SIZE_MAX) {
        prog[first_sq] |= LOP_PREFETCH | ((uint32_t)idx << 8);
        prog.push_back(op(LOP_B_READY, idx, 0, 0));
      } else {
        prog.push_back(loaded ? op(0, idx, 0, 0) : op(LOP_A_FROM_T, idx, first, 0));
      }
      loaded = true;
      first_sq = SIZE_MAX;
    }
  }
  if (!loaded) return false;
  prog.push_back(op(LOP_B_CONST | LOP_STORE, 0, 0, D4F_G));   // Z = Y' (1, 0)
  const std::vector<HBig> K = chain_weights(n, sched);
  kf.clear();
  for (int t = 0; t < LANE_NTILE; ++t) {
    const std::vector<uint32_t> l = mul_pow2_mod(K[t], RS, n).limbs(D4_S, LB);
    kf.insert(kf.end(), l.begin(), l.end());
  }
  return true;
}

// Op list of the factored 4096-bit decryption (d4f_run, kernels_dec4.hpp): the table's 30 one-pass products by the
// kept (A~, 0) (odd powers stored in tiles 0..15), the sliding-window chain over e = p_h - 2 with B-free multipliers,
// then Y' (A~, 0) (iota taken before it) and the product with (1, 0) into tile D4F_G. kf gets the closing sum's
// constants: K'_t = R sum over the chain's multiplies by entry t of 2^(squares after it) mod p_h, slot 0 = -R mod
// p_h (entry 1 is B-free, its slot carries the ciphertext's B_c term). tools/dec4f_model.py restates the algebra.
static bool build_dec4f_program(const HBig& ph, size_t RS, std::vector<uint32_t>& prog, std::vector<uint32_t>& kf) {
  const HBig e = sub(ph, HBig(2));
  if (e.bits() < 8) return false;
  std::vector<uint16_t> sched;
  int first = 0;
  sliding_schedule(e, sched, first);
  auto op = [](uint32_t flags, int bidx, int aidx, int sidx) {
    return flags | ((uint32_t)bidx << 8) | ((uint32_t)aidx << 16) | ((uint32_t)sidx << 24);
  };
  prog.clear();
  for (int t = 2; t < 2 * LANE_NTILE; ++t) prog.push_back(op(LOP_B_READY | ((t & 1) ? LOP_STORE : 0u), 0, 0, (t - 1) / 2));
  bool loaded = false;
  size_t first_sq = SIZE_MAX;
  for (size_t i = 0; i + 1 < sched.size(); i += 2) {
    const int nsq = sched[i], idx = sched[i + 1];
    for (int t = 0; t < nsq; ++t) {
      if (first_sq == SIZE_MAX) first_sq = prog.size();
      prog.push_back(loaded ? op(LOP_SQR, 0, 0, 0) : op(LOP_SQR | LOP_A_FROM_T, 0, first, 0));
      loaded = true;
    }
    if (idx != 0xFFFF) {
      if (first_sq != SIZE_MAX) {
        prog[first_sq] |= LOP_PREFETCH | ((uint32_t)idx << 8);
        prog.push_back(op(LOP_B_READY, idx, 0, 0));
      } else {
        prog.push_back(loaded ? op(0, idx, 0, 0) : op(LOP_A_FROM_T, idx, first, 0));
      }
      loaded = true;
      first_sq = SIZE_MAX;
    }
  }
  if (!loaded) return false;
  prog.push_back(op(LOP_IOTA, 0, 0, 0));                      // Z = Y' (A~, 0), A~ = tile 0's even component
  prog.push_back(op(LOP_B_CONST | LOP_STORE, 0, 0, D4F_G));   // (1 + p G) = Z (1, 0)
  const std::vector<HBig> K = chain_weights(ph, sched);
  kf.clear();
  for (int t = 0; t < LANE_NTILE; ++t) {
    const HBig v = t == 0 ? sub(ph, mul_pow2_mod(HBig(1), RS, ph)) : mul_pow2_mod(K[t], RS, ph);
    const std::vector<uint32_t> l = v.limbs(D4_S, LB);
    kf.insert(kf.end(), l.begin(), l.end());
  }
  return true;
}

template <typename K>
static int grid_for(pai_ctx* c, K kernel, size_t lds, long long units, int per_block) {
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, BLOCK, lds) != hipSuccess || occ < 1) occ = 1;
  long long want = (units + per_block - 1) / per_block;
  long long cap = (long long)occ * c->cus;
  return (int)std::max<long long>(1, std::min(want, cap));
}

static int ensure_scratch(pai_ctx* c, size_t bytes) {
  if (bytes <= c->scratch_bytes) return 0;
  if (c->d_scratch) HIPCHK(hipFree(c->d_scratch));
  c->d_scratch = nullptr;
  c->scratch_bytes = 0;
  HIPCHK(hipMalloc(&c->d_scratch, bytes));
  c->scratch_bytes = bytes;
  return 0;
}

static size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// hipMalloc that, when the device is full, first hands the released tables' pooled chunks (table_arena.hpp) back to the
// driver and tries again: pooled memory serves table rebuilds, never at the expense of a call's working buffers
static hipError_t dev_malloc(void** p, size_t bytes) {
  hipError_t e = hipMalloc(p, bytes);
  if (e == hipErrorOutOfMemory && TableArena::get().pooled_any()) {
    (void)hipGetLastError();
    TableArena::get().trim();
    e = hipMalloc(p, bytes);
  }
  return e;
}

static int ensure_buf(void** buf, size_t* have, size_t bytes) {
  if (bytes <= *have) return 0;
  if (*buf) HIPCHK(hipFree(*buf));
  *buf = nullptr;
  *have = 0;
  HIPCHK(dev_malloc(buf, bytes));
  *have = bytes;
  return 0;
}

static int ensure_work(pai_ctx* c, size_t bytes) {
  if (bytes <= c->work_bytes) return 0;
  if (c->d_work) HIPCHK(hipFree(c->d_work));
  c->d_work = nullptr;
  c->work_bytes = 0;
  HIPCHK(dev_malloc(&c->d_work, bytes));
  c->work_bytes = bytes;
  return 0;
}

static void stage_reset(pai_ctx* c) {
  if (c->stage_keep) return;   // inside a host-buffer call: its entry point reset once for all chunks
  c->nev = 0;
  c->nchunk_ev = 0;
}
// The events of a new chunk (nullptr when timing is off). The event table grows with the chunks of a call and is
// read only by pai_ctx_stage_times: recording a stage never waits on the device (folding the slots of a
// long call synchronised mid-call and removed the copy/compute overlap being timed).
static hipEvent_t* stage_chunk(pai_ctx* c) {
  if (!c->timing) return nullptr;
  if (c->nchunk_ev >= (int)c->ev.size()) c->ev.push_back({nullptr, nullptr, nullptr, nullptr});
  hipEvent_t* e = c->ev[c->nchunk_ev++].data();
  for (int i = 0; i < 4; ++i)
    if (!e[i]) (void)hipEventCreate(&e[i]);
  return e;
}
// mark i (0..3) of the current chunk; mark 0 opens a new chunk
static void stage_mark(pai_ctx* c, int i, hipStream_t st) {
  if (!c->timing || i >= 4) return;
  if (i == 0 && !stage_chunk(c)) return;
  if (c->nchunk_ev == 0) return;
  (void)hipEventRecord(c->ev[c->nchunk_ev - 1][i], st);
  c->nev = std::max(c->nev, i + 1);
}

template <typename K>
static int blocks_per_cu(K kernel, int threads, size_t lds) {
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, threads, lds) != hipSuccess || occ < 1) occ = 1;
  return occ;
}

// C-linkage comes from the declarations in flexpai.h.
const char* pai_last_error(void) { return g_last_error.c_str(); }

namespace fpai {
int set_error(int code, const char* msg) { return fail(code, msg); }   // for the other translation units
}

int pai_device_mem_info(int device, uint64_t* free_bytes, uint64_t* total_bytes) {
  HIPCHK(hipSetDevice(device));
  size_t fr = 0, tot = 0;
  HIPCHK(hipMemGetInfo(&fr, &tot));
  if (free_bytes) *free_bytes = fr;
  if (total_bytes) *total_bytes = tot;
  return 0;
}

int pai_device_count(int* count) {
  if (!count) return fail(PAI_ERR_ARG, "null argument");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    n = 0;
  }
  *count = n;
  return 0;
}

static int setup_pe(pai_ctx* c, const HBig& n);
static int setup_pe1(pai_ctx* c, const HBig& n);
static int setup_pe4(pai_ctx* c, const HBig& n);

int pai_ctx_create(const uint8_t* n_le, size_t n_bytes, int device, pai_ctx** out) {
  if (!n_le || !out || n_bytes == 0) return fail(PAI_ERR_ARG, "pai_ctx_create: null argument");
  SetupTrace tr("pai_ctx_create");
  HBig n = HBig::from_le_bytes(n_le, n_bytes);
  if (!n.is_odd() || n.bits() < 64) return fail(PAI_ERR_KEY, "pai_ctx_create: n must be odd and >= 64 bits");
  auto* c = new pai_ctx();
  c->device = device;
  c->counted = true;
  ++g_contexts;
  if (hipSetDevice(device) != hipSuccess) {
    delete c;
    return fail(PAI_ERR_HIP, "pai_ctx_create: hipSetDevice failed");
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
    delete c;
    return fail(PAI_ERR_HIP, "pai_ctx_create: hipGetDeviceProperties failed");
  }
  c->cus = prop.multiProcessorCount;
  c->n = n;
  c->nb = (int)n.bits();
  c->N = mul(n, n);
  c->tpi_e = tpi_for_bits(2 * (size_t)c->nb + 2, 2);
  c->tpi_d = tpi_for_bits((size_t)c->nb + 3, 1);
  if (!c->tpi_e || !c->tpi_d) {
    delete c;
    return fail(PAI_ERR_KEY, "pai_ctx_create: key size not supported (max 4096 bits)");
  }
  c->S_e = L * c->tpi_e;
  c->S_d = L * c->tpi_d;
  c->ct_words = (2 * c->nb + 31) / 32;
  c->pt_words = (c->nb + 31) / 32;
  c->mprime_N = mont_prime(c->N, LB);
  const size_t Rbits = (size_t)LB * c->S_e;
  HBig R2 = mul_pow2_mod(HBig(1), 2 * Rbits, c->N);
  std::vector<uint32_t> prog;
  if (!build_modexp_program(n, prog)) {
    delete c;
    return fail(PAI_ERR_KEY, "pai_ctx_create: degenerate exponent schedule");
  }
  c->nprog = (int)prog.size();
  HBig oneR = mul_pow2_mod(HBig(1), Rbits, c->N);
  std::vector<uint32_t> rs;
  {
    HMont M(c->N);
    HBig x(1);
    for (int s = 0; s <= ADD_KMAX + 1; ++s) {
      const std::vector<uint32_t> v = x.words(c->ct_words);
      rs.insert(rs.end(), v.begin(), v.end());
      x = M.mul(M.mul(x, oneR), M.r2);   // x R mod N
    }
  }
  int rc;
  if ((rc = upload(c, rs, &c->d_RS)) || (rc = upload(c, c->N.limbs(c->S_e, LB), &c->d_N)) ||
      (rc = upload(c, R2.limbs(c->S_e, LB), &c->d_R2)) ||
      (rc = upload(c, n.limbs(c->S_e, LB), &c->d_nl)) || (rc = upload(c, prog, &c->d_prog)) ||
      (rc = upload(c, oneR.limbs(c->S_e, LB), &c->d_oneR)) || (rc = (SetupTrace("  setup_pe"), setup_pe(c, n))) ||
      (rc = setup_pe1(c, n)) || (rc = setup_pe4(c, n))) {
    delete c;
    return rc;
  }
  if (c->S_e == 74 || c->S_e == 148 || c->S_e == 296) {   // public-key encryption of protocol-sized calls on rows (k_pe_w)
    std::vector<uint32_t> pw;
    if (build_lane_program(n, pw)) {
      if ((rc = upload(c, pw, &c->d_pew_prog))) {
        delete c;
        return rc;
      }
      c->pew_nprog = (int)pw.size();
    }
  }
#if FLEXPAI_XCHECK
  if (hipMalloc(&c->d_guard, sizeof(GuardRec)) != hipSuccess || hipMemset(c->d_guard, 0, sizeof(GuardRec)) != hipSuccess) {
    delete c;
    return fail(PAI_ERR_HIP, "pai_ctx_create: guard record");
  }
#endif
  *out = c;
  return 0;
}

// The test build's address guards (guard.hpp): the sizes the samplers' indices must stay below, as allocated here.
// $FLEXPAI_GUARD_INJECT=rows (test build only) passes a table of one row, so that every row index trips the guard:
// the self-test of the mechanism (tests/test_gpu_guard.py).
static GuardArgs guard_args(const pai_ctx* c, unsigned long long rows, unsigned long long digits, unsigned long long out,
                            unsigned long long in) {
  const char* inj = xcheck_env("FLEXPAI_GUARD_INJECT");
  if (inj && std::strcmp(inj, "rows") == 0) rows = 1;
  return GuardArgs{c->d_guard, rows, digits, out, in};
}
// after the guarded launches of a call: a violation fails the call with the first one's site, value and limit
static int guard_collect(pai_ctx* c, hipStream_t st) {
  if (!c->d_guard) return 0;
  HIPCHK(hipStreamSynchronize(st));
  GuardRec g{};
  HIPCHK(hipMemcpy(&g, c->d_guard, sizeof(g), hipMemcpyDeviceToHost));
  if (!g.hits) return 0;
  HIPCHK(hipMemset(c->d_guard, 0, sizeof(GuardRec)));
  return fail(PAI_ERR_HIP, std::string("address guard: ") + std::to_string(g.hits) + " violation(s), first at " +
                               guard_site_name(g.site) + ": index " + std::to_string(g.val) + " >= limit " +
                               std::to_string(g.lim) + " (element " + std::to_string(g.elem) + ")");
}

// Fixed-base obfuscation setup (kernels_fb.hpp): the smallest g >= 2 that generates Z_P* as far as
// the prime factors of P - 1 below 2^24 can tell (g^((P-1)/l) != 1 for each); a prime factor l of
// P - 1 above the bound that g misses has probability about 1/l < 2^-24. G = g^n mod P^2.
constexpr uint32_t FB_TRIAL_BOUND = 1u << 24;   // = oracle/paillier_oracle.py FB_TRIAL_BOUND

// The primes below FB_TRIAL_BOUND in chunks of 4096 with each chunk's product (a product tree on GMP), built once
// per process: the small prime factors of P - 1 are then found chunk by chunk as gcd(prod_j mod (P - 1), P - 1)
// (~0.3 k GMP operations per key instead of 1.08 M single-precision remainders: 66 -> a few ms per half, round 5).
struct PrimeChunks {
  std::vector<uint32_t> primes;
  std::vector<size_t> start;                  // chunk j = primes[start[j] .. start[j + 1])
  std::vector<std::unique_ptr<Mpz>> prod;
};
static void prime_product(const std::vector<uint32_t>& pr, size_t lo, size_t hi, mpz_t out) {
  if (hi - lo <= 16) {
    mpz_set_ui(out, 1);
    for (size_t i = lo; i < hi; ++i) mpz_mul_ui(out, out, pr[i]);
    return;
  }
  const size_t mid = (lo + hi) / 2;
  Mpz a, b;
  prime_product(pr, lo, mid, a.v);
  prime_product(pr, mid, hi, b.v);
  mpz_mul(out, a.v, b.v);
}
static const PrimeChunks& prime_chunks() {
  static const PrimeChunks pc = [] {
    PrimeChunks c;
    c.primes = small_primes(FB_TRIAL_BOUND);
    constexpr size_t CH = 4096;
    for (size_t s = 0; s < c.primes.size(); s += CH) {
      c.start.push_back(s);
      c.prod.emplace_back(new Mpz());
      prime_product(c.primes, s, std::min(s + CH, c.primes.size()), c.prod.back()->v);
    }
    c.start.push_back(c.primes.size());
    return c;
  }();
  return pc;
}

static uint32_t fb_base(const HBig& P) {
  const PrimeChunks& pc = prime_chunks();
  Mpz p(P), pm1, t, g;
  mpz_sub_ui(pm1.v, p.v, 1);
  std::vector<uint32_t> fac;
  for (size_t j = 0; j < pc.prod.size(); ++j) {
    mpz_mod(t.v, pc.prod[j]->v, pm1.v);
    mpz_gcd(g.v, t.v, pm1.v);
    if (mpz_cmp_ui(g.v, 1) == 0) continue;
    for (size_t i = pc.start[j]; i < pc.start[j + 1]; ++i)
      if (mpz_divisible_ui_p(g.v, pc.primes[i])) fac.push_back(pc.primes[i]);
  }
  std::vector<std::unique_ptr<Mpz>> cof;
  for (uint32_t l : fac) {
    cof.emplace_back(new Mpz());
    mpz_divexact_ui(cof.back()->v, pm1.v, l);
  }
  Mpz gb, r;
  for (uint32_t cand = 2; cand < 1000000u; ++cand) {
    bool ok = true;
    for (size_t k = 0; k < fac.size() && ok; ++k) {
      if (fac[k] == 2) {   // g^((P-1)/2) == 1 iff g is a square mod P (Euler's criterion)
        mpz_set_ui(gb.v, cand);
        ok = mpz_jacobi(gb.v, p.v) != 1;
      } else {
        mpz_set_ui(gb.v, cand);
        mpz_powm(r.v, gb.v, cof[k]->v, p.v);
        ok = mpz_cmp_ui(r.v, 1) != 0;
      }
    }
    if (ok) return cand;
  }
  return 0;
}


// Public-key encryption on split pairs (kernels_pe.hpp) for n of 1537..2048 bits: S = 74 limbs of n, R =
// 2^(28 S) >= 2^24 n. Constants: n, (1 - R) and (1 - R^2) mod n, the pair of R^3 mod n^2, the op list for n.
static int setup_pe(pai_ctx* c, const HBig& n) {
  bool pair = true;
  if (const char* e = xcheck_env("FLEXPAI_PAIR")) pair = atoi(e) != 0;
  const size_t RS = (size_t)LB * D4_S;
  if (!pair || n.bits() + 24 > RS || n.bits() <= 1536) return 0;
  std::vector<uint32_t> prog;
  if (!build_lane_program(n, prog)) return 0;
  const HBig n2 = mul(n, n);
  auto one_minus = [&](const HBig& r) { return mod(sub(add(n, HBig(1)), r), n); };   // (1 - r) mod n, 0 < r < n
  const HBig r3 = mul_pow2_mod(HBig(1), 3 * RS, n2);
  const HBig qt = div_big(r3, n), rm = sub(r3, mul(qt, n));
  std::vector<uint32_t> ck = rm.limbs(D4_S, LB), b = qt.limbs(D4_S, LB);
  ck.insert(ck.end(), b.begin(), b.end());
  uint32_t *dn, *dx1, *dxk, *dck, *dprog;
  int rc;
  if ((rc = upload(c, n.limbs(D4_S, LB), &dn)) ||
      (rc = upload(c, one_minus(mul_pow2_mod(HBig(1), RS, n)).limbs(D4_S, LB), &dx1)) ||
      (rc = upload(c, one_minus(mul_pow2_mod(HBig(1), 2 * RS, n)).limbs(D4_S, LB), &dxk)) ||
      (rc = upload(c, ck, &dck)) || (rc = upload(c, prog, &dprog)))
    return rc;
  std::vector<PeConst> pc{PeConst{dn, dx1, dxk, dck, dprog, (int)prog.size(), mont_prime(n, LB)}};
  // the factored chain (kernels_pe.hpp k_pe_pow_f): its program and Horner weights, R^2 mod n; R mod n for the batch
  // inversion of the bases mod n on the TPI = 2 group engine (same radix R = 2^(28 74))
  std::vector<uint32_t> progf, kf;
  const bool pef = !(xcheck_env("FLEXPAI_PEF") && atoi(xcheck_env("FLEXPAI_PEF")) == 0);
  if (pef && tpi_for_bits((size_t)c->nb + 3, 1) == 2 && build_pef_program(n, RS, progf, kf)) {
    uint32_t *dpf, *dkf, *dr2, *done;
    if ((rc = upload(c, progf, &dpf)) || (rc = upload(c, kf, &dkf)) ||
        (rc = upload(c, mul_pow2_mod(HBig(1), 2 * RS, n).limbs(D4_S, LB), &dr2)) ||
        (rc = upload(c, mul_pow2_mod(HBig(1), RS, n).limbs(D4_S, LB), &done)))
      return rc;
    pc[0].progf = dpf;
    pc[0].nprogf = (int)progf.size();
    pc[0].kf = dkf;
    pc[0].r2n = dr2;
    c->d_pe_n = dn;
    c->d_pe_r2 = dr2;
    c->d_pe_oneR = done;
    c->pe_mprime = mont_prime(n, LB);
    c->pef_ok = true;
  }
  if ((rc = upload(c, pc, &c->d_pe))) return rc;
  c->pe_ok = true;
  return 0;
}

// Public-key encryption on pairs over the S = 37 limbs of n for n <= 1024 bits (kernels_pe1.hpp; R = 2^1036 >= 2^12 n):
// n, the pair of R^3 mod n^2 (r's two digit chunks, k_dec_pre_pair), the pair (1, 0), the op list over n, R^2 mod n.
static int setup_pe1(pai_ctx* c, const HBig& n) {
  bool pair = true;
  if (const char* e = xcheck_env("FLEXPAI_PAIR")) pair = atoi(e) != 0;
  const size_t RS = (size_t)LB * PE1_S;
  if (!pair || n.bits() + 12 > RS || c->ct_words > 64) return 0;
  std::vector<uint32_t> prog;
  if (!build_lane_program(n, prog)) return 0;
  const HBig n2 = mul(n, n);
  const HBig r3 = mul_pow2_mod(HBig(1), 3 * RS, n2);
  const HBig qt = div_big(r3, n), rm = sub(r3, mul(qt, n));
  std::vector<uint32_t> ck = rm.limbs(PE1_S, LB), b = qt.limbs(PE1_S, LB), one(2 * PE1_S, 0);
  ck.insert(ck.end(), b.begin(), b.end());
  one[0] = 1;
  uint32_t *dn, *dck, *done, *dprog, *dr2;
  int rc;
  if ((rc = upload(c, n.limbs(PE1_S, LB), &dn)) || (rc = upload(c, ck, &dck)) || (rc = upload(c, one, &done)) ||
      (rc = upload(c, prog, &dprog)) || (rc = upload(c, mul_pow2_mod(HBig(1), 2 * RS, n).limbs(PE1_S, LB), &dr2)))
    return rc;
  const uint32_t mp = mont_prime(n, LB);
  std::vector<DecPairHalf> h{DecPairHalf{dn, dck, nullptr, nullptr, mp, 0u}};
  if ((rc = upload(c, h, &c->d_pe1_half))) return rc;
  c->d_pe1_n = dn;
  c->d_pe1_one = done;
  c->d_pe1_prog = dprog;
  c->pe1_nprog = (int)prog.size();
  c->d_pe1_r2n = dr2;
  c->pe1_mprime = mp;
  c->pe1_ok = true;
  return 0;
}

// Public-key encryption on pair groups (kernels_pe4.hpp) for n of 2049..4096 bits: S = 152 limbs of n, R = 2^(28 S)
// >= 2^24 n. Constants: n, (1 - R) and (1 - R^2) mod n, the pair of R^3 mod n^2, the op list for n; for k_pe4_fin
// n^2 and n R' mod n^2 on the 296 limbs of the L = 37 group engine (R' = 2^(28 296)).
static int setup_pe4(pai_ctx* c, const HBig& n) {
  bool pair = true;
  if (const char* e = xcheck_env("FLEXPAI_PAIR")) pair = atoi(e) != 0;
  const size_t RS = (size_t)LB * PE4_S;
  if (!pair || n.bits() <= 2048 || n.bits() > 4096 || n.bits() + 24 > RS || c->ct_words > 2 * PE4_S) return 0;
  std::vector<uint32_t> prog;
  if (!build_lane_program(n, prog)) return 0;
  const HBig n2 = mul(n, n);
  auto one_minus = [&](const HBig& r) { return mod(sub(add(n, HBig(1)), r), n); };   // (1 - r) mod n, 0 < r < n
  const HBig r3 = mul_pow2_mod(HBig(1), 3 * RS, n2);
  const HBig qt = div_big(r3, n), rm = sub(r3, mul(qt, n));
  std::vector<uint32_t> ck = rm.limbs(PE4_S, LB), b = qt.limbs(PE4_S, LB);
  ck.insert(ck.end(), b.begin(), b.end());
  uint32_t *dn, *dx1, *dxk, *dck, *dprog, *dn2, *dnr;
  int rc;
  if ((rc = upload(c, n.limbs(PE4_S, LB), &dn)) ||
      (rc = upload(c, one_minus(mul_pow2_mod(HBig(1), RS, n)).limbs(PE4_S, LB), &dx1)) ||
      (rc = upload(c, one_minus(mul_pow2_mod(HBig(1), 2 * RS, n)).limbs(PE4_S, LB), &dxk)) ||
      (rc = upload(c, ck, &dck)) || (rc = upload(c, prog, &dprog)) || (rc = upload(c, n2.limbs(PE4_FS, LB), &dn2)) ||
      (rc = upload(c, mul_pow2_mod(n, (size_t)LB * PE4_FS, n2).limbs(PE4_FS, LB), &dnr)))
    return rc;
  std::vector<Pe4Const> pc{Pe4Const{dn, dx1, dxk, dck, dprog, (int)prog.size(), mont_prime(n, LB), dn2, dnr, mont_prime(n2, LB)}};
  if ((rc = upload(c, pc, &c->d_pe4))) return rc;
  c->pe4_ok = true;
  return 0;
}

// Split-pair sampler (kernels_sgp.hpp) over the pair-group tables of modulus P (rows T R, R = 2^(28 FBGP_S)): C =
// 2^(-56 K) mod P^2 as (C mod P, C div P), the chunk weights w 2^(16 c) C_A mod P of c0 = (1, w |M|), and 2^20 P.
// FLEXPAI_SGP=0 keeps the group-engine samplers (k_fbgp, k_pfb).
static bool sgp_enabled() {
  const char* e = xcheck_env("FLEXPAI_SGP");
  return !e || atoi(e) != 0;
}
// Shoup rows for the 4096-bit key holder's split-pair sampler (kernels_sgs.hpp). Their 640-B rows sit beside the
// factored rows (whose b halves they keep using): 1152 B per entry against 512, so they fit one window lower (W = 20
// at nb = 4096 on a 288-GB device, 249 GB, against the factored rows' W = 21, 205 GB). fb_choose takes them when the
// product count at their window, priced at the measured 0.835 of a Montgomery row product
// (profiles/r05_ab_sgs_prototype_stream.txt), is below the factored rows' at theirs. $FLEXPAI_SGS=0 never takes them,
// $FLEXPAI_SGS=1 whenever they fit.
static int sgs_mode() {
  const char* e = getenv("FLEXPAI_SGS");
  return !e || !*e ? -1 : atoi(e) != 0 ? 1 : 0;
}
// Garner's last step on lanes (k_sgp_fin); the test build's $FLEXPAI_SGP_FIN=0 keeps the group kernel k_fbg_fin
static bool sgp_fin_enabled() {
  const char* e = xcheck_env("FLEXPAI_SGP_FIN");
  return !e || atoi(e) != 0;
}

static int sgp_make_half(const HBig& P, const HBig& w, int K, const void* table, std::vector<void*>& mem, SgpHalf* out) {
  const HBig P2 = mul(P, P);
  const HBig C = inv_mod(mul_pow2_mod(HBig(1), (size_t)LB * (FBGP_S - SGP_S) * K, P2), P2);
  if (C.is_zero()) return fail(PAI_ERR_KEY, "split-pair sampler: 2 not invertible mod P^2");
  const HBig cb = div_big(C, P), ca = sub(C, mul(cb, P));
  std::vector<uint32_t> nmc;
  for (int k = 0; k < 4; ++k) append(nmc, mod(mul(mul_pow2_mod(mod(w, P), (size_t)16 * k, P), ca), P).limbs(SGP_S, LB));
  uint32_t *dp, *dca, *dcb, *dnmc, *dpb;
  int rc;
  if ((rc = upload_to(mem, P.limbs(SGP_S, LB), &dp)) || (rc = upload_to(mem, ca.limbs(SGP_S, LB), &dca)) ||
      (rc = upload_to(mem, cb.limbs(SGP_S, LB), &dcb)) || (rc = upload_to(mem, nmc, &dnmc)) ||
      (rc = upload_to(mem, mul(P, pow2(20)).limbs(SGP_S, LB), &dpb)))
    return rc;
  *out = SgpHalf{(const uint4*)table, dp, dca, dcb, dnmc, dpb, mont_prime(P, LB)};
  return 0;
}

// The Shoup rows of both halves from their factored rows t[h] (kernels_sgs.hpp k_sgs_conv) and the constants of
// k_sgs_bfin: w 2^(16 c) R mod P (R = 2^(28 FBGP_S), the b rows' radix; w = the other prime) and mu = floor(2^(56 S) / P).
// The row memory at[h] was reserved before the factored tables were built (ensure_fb), so that a device without room for
// both never ends up on the factored rows at the Shoup rows' lower window. Any failure here leaves the Montgomery sampler
// k_sgp in place over the complete factored tables (returns nonzero with the reason in pai_last_error; the caller frees
// at[] and keeps the fixed-base path).
static int sgs_build(pai_ctx* c, const HBig* primes, int K, int W, void* const* t, const SgpHalf* sv, uint4* const* at) {
  SgsHalf sh[2];
  const size_t rows = (size_t)K << W;
  for (int h = 0; h < 2; ++h) {
    const HBig& P = primes[h];
    std::vector<uint32_t> nmr;
    for (int k = 0; k < 4; ++k)
      append(nmr, mul_pow2_mod(mod(primes[1 - h], P), (size_t)16 * k + (size_t)LB * FBGP_S, P).limbs(SGP_S, LB));
    const HBig mu = div_big(pow2((size_t)2 * LB * SGP_S), P);
    if (mu.bits() > (size_t)LB * (SGP_S + 1)) return fail(PAI_ERR_KEY, "Shoup rows: mu exceeds S + 1 limbs");
    // R^-K mod P^2 = c_A (1 + P beta): the rows' Montgomery factor R = 2^(28 FBGP_S), once per row product
    const HBig P2 = mul(P, P);
    const HBig Ci = inv_mod(mul_pow2_mod(HBig(1), (size_t)LB * FBGP_S * K, P2), P2);
    if (Ci.is_zero()) return fail(PAI_ERR_KEY, "Shoup rows: 2 not invertible mod P^2");
    const HBig cB = div_big(Ci, P), cA = sub(Ci, mul(cB, P));
    const HBig cAi = inv_mod(cA, P);
    if (cAi.is_zero()) return fail(PAI_ERR_KEY, "Shoup rows: c_A not invertible");
    // the pass multiplies by the integer y = c_A R' mod P, and y R'^-1 = c_A (1 + P delta)^-1 mod P^2 with Y = c_A R'
    // mod P^2 = y (1 + P delta): delta joins the b sum with beta
    const HBig Y = mul_pow2_mod(cA, (size_t)LB * SGP_S, P2);
    const HBig yB = div_big(Y, P), y = sub(Y, mul(yB, P));
    const HBig yi = inv_mod(y, P);
    if (yi.is_zero()) return fail(PAI_ERR_KEY, "Shoup rows: y not invertible");
    const HBig delta = mod(mul(yB, yi), P);
    const HBig beta = mod(add(mul(cB, cAi), delta), P);
    uint32_t *dn, *dmu, *dcy, *dbr;
    int rc;
    std::vector<void*>& mem = c->fb.mem;
    if ((rc = upload_to(mem, nmr, &dn)) || (rc = upload_to(mem, mu.limbs(SGP_S + 2, LB), &dmu)) ||
        (rc = upload_to(mem, y.words(FBGP_PW), &dcy)) ||
        (rc = upload_to(mem, mul_pow2_mod(beta, (size_t)LB * FBGP_S, P).limbs(SGP_S, LB), &dbr)))
      return rc;
    sh[h] = SgsHalf{at[h], (const uint4*)t[h], sv[h].p, dn, sv[h].pbig, dmu, dcy, dbr, sv[h].mprime};
  }
  SgsHalf* d = nullptr;
  std::vector<SgsHalf> shv(sh, sh + 2);
  int rc;
  if ((rc = upload_to(c->fb.mem, shv, &d))) return rc;
  if (sgs_launch_conv(d, rows, at[0], at[1], nullptr) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    (void)hipGetLastError();
    return fail(PAI_ERR_HIP, "Shoup row conversion failed");
  }
  c->fb.d_sgs = d;
  return 0;
}

// Digit windows the table builder supports (lo/hi half-digit tables of at most FB_LO entries)
static bool fb_window_ok(int w) { return w == 8 || w == 12 || w == 16 || (w >= 20 && w <= 24); }

// g_contexts, g_key_holders (above): contexts of this process, and those holding a private key.
static bool fb_window_auto() {
  const char* e = getenv("FLEXPAI_FB_WINDOW");
  return e && strcmp(e, "auto") == 0;
}

// Window of the key holder's tables: $FLEXPAI_FB_WINDOW, default 16 (2 x 1.07 GB at nb = 2048: a process may hold
// several keys). "auto": a process whose only private key is this one asks for the largest window (24) and
// gets the largest whose tables fit auto's share of the free HBM (fb_budget), i.e. W = 22 at nb = 2048 (2 x 88.3 GB of
// 448-B Shoup rows) and W = 21 at nb = 4096 on an otherwise empty MI355X; a process holding several keys gets 16.
static int fb_default_window() {
  if (fb_window_auto()) return g_key_holders.load() <= 1 ? 24 : 16;
  const char* e = getenv("FLEXPAI_FB_WINDOW");
  const int w = e ? atoi(e) : 16;
  return fb_window_ok(w) ? w : 16;
}

// Windows of the public-key tables: the ones pinned to reference goldens (12, 16, 20; tests/golden/
// make_golden_pfb.py). Their K = K0 + 32 KS rows keep k_sgp's b sum within its bound (K <= 512; W = 8 would
// need 648). "auto": 20 for a process with one context, else 16.
static bool pfb_window_ok(int w) { return w == 12 || w == 16 || w == 20; }

static int pfb_default_window() {
  if (fb_window_auto()) return g_contexts.load() <= 1 ? 20 : 16;
  const char* e = getenv("FLEXPAI_FB_WINDOW");
  const int w = e ? atoi(e) : 16;
  return pfb_window_ok(w) ? w : w > 20 ? 20 : 16;
}

// 32-bit words of one table row: packed words for the lane kernels, S canonical limbs for the group kernel
static int fb_row_words(int sb) {
  return sb == 37 ? FbGeom<37>::TW : sb == 74 ? FbGeom<74>::TW : sb == GRP_TPI * L ? GRP_TPI * L : 0;
}

// 4096-bit keys: the pair-group sampler (kernels_grp_pair.hpp) runs when both p_h fit its 76 limbs with
// R >= 2^24 p_h; its rows are the canonical pair as 2 x 64 words
static bool fb_gpair_possible(const pai_ctx* c) {
  if (c->crt_sb != GRP_TPI * L) return false;
  for (const HBig* h : {&c->fb_p, &c->fb_q})
    if (h->bits() + 24 > (size_t)LB * FBGP_S || h->bits() > (size_t)LB * FBGP_SP || h->bits() > (size_t)32 * FBGP_PW)
      return false;
  return true;
}

static int fb_row_words(const pai_ctx* c) { return fb_gpair_possible(c) ? 4 * FBGP_ROW4 : fb_row_words(c->crt_sb); }

// 1024/2048-bit keys: the pair tables (kernels_fbp.hpp) need p_h < 2^(32 PW) and R = 2^(28 S) >= 2^12 p_h (bounds of
// the first product, kernels_fbp.hpp). Returns S (19 or 37), or 0.
static int fb_pair_possible(const pai_ctx* c) {
  const int sb = c->crt_sb;
  const int ps = sb == 37 ? 19 : sb == 74 ? 37 : 0;
  if (!ps) return 0;
  const int pw = ps == 19 ? FbpGeom<19>::PW : FbpGeom<37>::PW;
  for (const HBig* h : {&c->fb_p, &c->fb_q})
    if (h->bits() > (size_t)32 * pw || h->bits() + FBP_PB + 1 > (size_t)LB * ps) return 0;
  return ps;
}

// Shoup rows (kernels_fbs.hpp, k_fbs) on the pair path: the product's sampler for 1024/2048-bit keys. The test build
// keeps k_fbp's Montgomery rows behind $FLEXPAI_FBS=0 for the cross-checks. Shoup's a' = floor(a R / p_h) < R and
// k_fbs_fill's mu = floor(R^2 / p_h) must fit S + 1 limbs: p_h > 2^(28 (S - 1)).
static bool fb_shoup_possible(const pai_ctx* c) {
  const int ps = fb_pair_possible(c);
  if (!ps) return false;
  const char* e = xcheck_env("FLEXPAI_FBS");
  if (e && atoi(e) == 0) return false;
  for (const HBig* h : {&c->fb_p, &c->fb_q})
    if (h->bits() <= (size_t)LB * (ps - 1)) return false;
  return true;
}

// 32-bit words of one resident table row (fb_row_words is the ciphertext half's word count for the Garner
// kernels; the Shoup rows are longer: a, a', b R)
static int fb_table_row_words(const pai_ctx* c) {
  if (fb_shoup_possible(c)) return fbs_row_bytes(fb_pair_possible(c)) / 4;
  return fb_row_words(c);
}

// bits of the exponents a_h < p_h - 1
static int fb_exponent_bits(const pai_ctx* c) {
  return (int)std::max(sub(c->fb_p, HBig(1)).bits(), sub(c->fb_q, HBig(1)).bits());
}

static int fb_digit_count(const pai_ctx* c, int W) { return fb_cut_uniform(fb_exponent_bits(c), W).K; }

static uint64_t fb_bytes(const pai_ctx* c, int W, bool sgs = false) {
  return 2ull * (uint64_t)fb_digit_count(c, W) * (1ull << W) * ((uint64_t)fb_table_row_words(c) + (sgs ? 4ull * SGS_ROW_Q : 0ull)) *
         4ull;
}

// The window of the tables (<= c->fb_W, within budget) and whether Shoup rows join them (sgs_mode, above)
static int fb_choose(const pai_ctx* c, uint64_t budget, bool* sgs, bool allow_sgs = true) {
  static const int ladder[] = {24, 23, 22, 21, 20, 16, 12, 8};
  const int wm = fb_ladder_window(fb_exponent_bits(c), c->fb_W, 4ull * fb_table_row_words(c), budget);
  int ws = 0;
  const int mode = allow_sgs ? sgs_mode() : 0;
  if (mode != 0 && fb_gpair_possible(c) && sgp_enabled())
    for (int w : ladder)
      if (w <= c->fb_W && fb_bytes(c, w, true) <= budget) {
        ws = w;
        break;
      }
  *sgs = ws && (mode == 1 || (wm && 0.835 * fb_digit_count(c, ws) < (double)fb_digit_count(c, wm)));
  return *sgs ? ws : wm;
}

// Budget for the two tables: $FLEXPAI_FB_MAX_BYTES, else the free device memory less a reserve of
// max(4 GiB, 1/12 of the device) -- 24 GB on a 288 GB MI355X -- kept for what the context (and others in
// the process) allocate after the tables: host-pipeline buffers for larger calls, decryption work and
// scratch, k_add's schedule, a configs[3] shard with its all-gather receive buffers.
// With FLEXPAI_FB_WINDOW=auto the budget is further capped at $FLEXPAI_FB_AUTO_FRAC (default 0.75) of the free
// memory, so an automatic choice never takes the whole device (W = 22 at nb = 2048 is 177 GB of 287 GB free; W = 23's
// Shoup rows, 338 GB, do not fit).
static uint64_t fb_budget(const pai_ctx* c) {
  if (const char* e = getenv("FLEXPAI_FB_MAX_BYTES")) return (uint64_t)strtod(e, nullptr);
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) return 0;
  fr += TableArena::get().pooled_bytes(c->device);   // released tables' chunks, held for reuse (table_arena.hpp)
  const uint64_t reserve = std::max<uint64_t>(4ull << 30, (uint64_t)tot / 12);
  uint64_t b = fr > reserve ? fr - reserve : 0;
  if (fb_window_auto()) {
    const char* f = getenv("FLEXPAI_FB_AUTO_FRAC");
    double frac = f ? atof(f) : 0.75;
    if (!(frac > 0.0 && frac <= 1.0)) frac = 0.75;
    b = std::min<uint64_t>(b, (uint64_t)(frac * (double)fr));
  }
  return b;
}

// Fixed-base break-even: the tables cost a one-time build (host bases + k_fb*_lohi/fill over 2 K 2^W rows,
// ~2.1 ns per 256-B row on one MI355X, profiles/r02_bench_v13.log setup) and save, per element, the
// difference between the generic path and the sampler (nb = 2048: 1/1.63 M - 1/40 M s = 0.59 us; nb = 4096
// against the public-key kernel: 1/37 k - 1/4.2 M s = 27 us; nb = 1024: ~0.08 us). A fresh key builds them
// only once the device-RNG elements of this context (this call included) reach the break-even count --
// a re-keying caller (HE_SA_FT, he_sa_ft/train.py:39-40) encrypting a few hundred elements per key never
// pays the build. $FLEXPAI_FB_MIN_ELEMS overrides the count; pai_ctx_fixed_base_prepare builds at once.
static long long fb_break_even(const pai_ctx* c, uint64_t rows, int row_bytes) {   // rows: per half
  if (const char* e = getenv("FLEXPAI_FB_MIN_ELEMS")) return atoll(e);
  const double build_s = 0.05 + 2.0 * (double)rows * 2.1e-9 * (row_bytes / 256.0);
  const double save_s = c->nb > 2048 ? 27e-6 : c->nb > 1024 ? 0.59e-6 : 0.08e-6;
  return (long long)(build_s / save_s) + 1;
}

static bool fb_wanted(pai_ctx* c, long long n);
static bool pfb_supported(const pai_ctx* c);

static int fb_unavailable(pai_ctx* c, const std::string& why) {
  c->fb.release();
  (void)hipGetLastError();   // clear a failed allocation / launch so later calls start clean
  c->fb_state = pai_ctx::FB_UNAVAILABLE;
  c->fb_reason = why;
  static bool warned = false;
  if (!warned && !getenv("FLEXPAI_QUIET")) {
    fprintf(stderr, "flexpai: fixed-base obfuscation unavailable (%s); encrypting through the generic CRT path\n",
            why.c_str());
    warned = true;
  }
  return 0;
}

// 28-bit limbs (device) -> HBig
static HBig from_limbs(const uint32_t* l, int nl) {
  HBig r;
  r.w.assign(((size_t)nl * LB + 31) / 32 + 2, 0);
  for (int i = 0; i < nl; ++i) {
    const size_t bit = (size_t)LB * i;
    const uint64_t v = (uint64_t)l[i] << (bit % 32);
    r.w[bit / 32] |= (uint32_t)v;
    r.w[bit / 32 + 1] |= (uint32_t)(v >> 32);
  }
  r.trim();
  return r;
}

// The host step of the factored rows' batch inversion (kernels_grp_pair.hpp): the nv chain products v_i
// (R-forms, < 2m, S limbs each at d_cval) -> v_i^-1 R_dev^2 mod m, R_dev = 2^(28 S), in place. Montgomery's
// trick over the nv values and one binary extended-Euclid inversion: m may be composite (n).
static int pair_host_invert(const HBig& m, uint32_t* d_cval, int nv, int S) {
  std::vector<uint32_t> buf((size_t)nv * S);
  HIPCHK(hipMemcpy(buf.data(), d_cval, buf.size() * 4, hipMemcpyDeviceToHost));
  HMont M(m);
  std::vector<HBig> xm(nv), pre(nv);
  for (int i = 0; i < nv; ++i) {
    HBig v = from_limbs(&buf[(size_t)i * S], S);
    while (cmp(v, m) >= 0) v = sub(v, m);
    if (v.is_zero()) return fail(PAI_ERR_KEY, "table construction: a zero chain product");
    xm[i] = M.mul(v, M.r2);                       // host Montgomery form
    pre[i] = i ? M.mul(pre[i - 1], xm[i]) : xm[i];
  }
  const HBig ti = inv_mod(M.from(pre[nv - 1]), m);
  if (ti.is_zero()) return fail(PAI_ERR_KEY, "table construction: a chain product is not invertible");
  const HBig rdm = M.mul(mul_pow2_mod(HBig(1), 2 * (size_t)LB * S, m), M.r2);   // R_dev^2, host Montgomery form
  HBig I = M.mul(ti, M.r2);
  for (int i = nv - 1; i >= 0; --i) {
    const HBig inv = i ? M.mul(I, pre[i - 1]) : I;
    if (i) I = M.mul(I, xm[i]);
    const std::vector<uint32_t> l = M.from(M.mul(inv, rdm)).limbs(S, LB);
    std::copy(l.begin(), l.end(), buf.begin() + (size_t)i * S);
  }
  HIPCHK(hipMemcpy(d_cval, buf.data(), buf.size() * 4, hipMemcpyHostToDevice));
  return 0;
}

// Device scratch of one modulus's factored-row build (kernels_fbp.hpp, kernels_grp_pair.hpp, kernels_pfb.hpp), sized from
// the digit positions K, the window W and the limbs S of the modulus; freed with the object.
struct RowScratch {
  uint32_t* lohi = nullptr;    // [K][2][FB_LO][2S] lo/hi half-digit entries
  uint32_t* inv = nullptr;     // [K][2][FB_LO][S] inverses of their A parts
  uint32_t* pre = nullptr;     // [2K][2^(W - W/2)][S] the batch inversion's prefix products
  uint32_t* cval = nullptr;    // [2K][S] the chain products, then their inverses (pair_host_invert)
  uint32_t* bases = nullptr;   // [K][2][2S] the public tables' digit bases (a key holder uploads its own)
  RowScratch() = default;
  RowScratch(const RowScratch&) = delete;
  RowScratch& operator=(const RowScratch&) = delete;
  ~RowScratch() { free(); }
  bool alloc(int K, int W, int S, bool with_bases = false) {
    const size_t e = (size_t)S * 4, k = (size_t)K;
    return hipMalloc(&lohi, k * 2 * FB_LO * 2 * e) == hipSuccess && hipMalloc(&inv, k * 2 * FB_LO * e) == hipSuccess &&
           hipMalloc(&pre, (2 * k << (W - W / 2)) * e) == hipSuccess && hipMalloc(&cval, 2 * k * e) == hipSuccess &&
           (!with_bases || hipMalloc(&bases, k * 2 * 2 * e) == hipSuccess);
  }
  void free() {
    for (uint32_t** p : {&lohi, &inv, &pre, &cval, &bases}) {
      if (*p) (void)hipFree(*p);
      *p = nullptr;
    }
  }
};

// The factored rows of nmod moduli (S limbs each, K digit positions): phase 1 (the lo/hi entries and the batch inversion's
// forward pass), the host inversion of each modulus's 2K chain products, phase 2 (backward pass, fill). lab: the setup
// trace's labels of phase 1, of the inversion (null: timed with phase 1) and of phase 2. The reason of a failure is in
// pai_last_error.
template <class Phase1, class Phase2>
static int build_factored_rows(const char* const (&lab)[3], Phase1&& phase1, Phase2&& phase2, const HBig* mods,
                               const RowScratch* sc, int nmod, int K, int S) {
  {
    std::optional<SetupTrace> tr(std::in_place, lab[0]);
    if (phase1() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(PAI_ERR_HIP, "table construction failed");
    if (lab[1]) tr.emplace(lab[1]);
    for (int h = 0; h < nmod; ++h)
      if (int rc = pair_host_invert(mods[h], sc[h].cval, 2 * K, S)) return rc;
  }
  SetupTrace tr(lab[2]);
  if (phase2() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(PAI_ERR_HIP, "table construction failed");
  return 0;
}

// What ensure_fb builds for this key within the memory budget: the sampler family, the window and the digit geometry.
// why: the first check that refuses the key, in ensure_fb's order (null: the key is accepted). The window is chosen
// whenever one fits, whatever the later checks say, so that fb_threshold prices the very build ensure_fb would start.
struct FbPlan {
  const char* why = nullptr;
  int sb = 0;            // limbs of p_h^2 (crt_sb)
  bool grp = false;      // 4096-bit keys: halves of 148 limbs, recombined by the group-engine Garner kernels
  int ps = 0;            // 1024/2048-bit keys: pairs over the ps = 19 / 37 limbs of p_h (kernels_fbp.hpp)
  bool shoup = false;    //   ... on Shoup rows (kernels_fbs.hpp); the product takes nothing else
  bool gpair = false;    // 4096-bit keys: pair groups (kernels_grp_pair.hpp)
  bool sgp = false;      //   ... with the split-pair sampler's constants (kernels_sgp.hpp); the product takes nothing else
  bool sgs = false;      //   ... and Shoup rows beside the factored rows (kernels_sgs.hpp; fb_choose)
  int S = 0;             // limbs of a pair's components: ps, or FBGP_S
  int row_words = 0;     // 32-bit words of one resident row (without the 4096-bit Shoup rows)
  int W = 0, K = 0, raw_bits = 0;
  int nw = 0;            // Shoup rows: the first nw of the K digits hold W + 1 bits (fb_cut.hpp); 0: the uniform cut
  size_t rows() const { return (size_t)fb_cut_row(K, W, nw); }   // per half
};

static FbPlan fb_plan(pai_ctx* c, bool allow_sgs = true) {
  FbPlan pl;
  auto refuse = [&pl](const char* why) {
    pl.why = why;
    return pl;
  };
  if (!c->crt_ok && !c->fbg_ok) return refuse("needs the private key and the CRT kernels");
  const int TW = fb_row_words(c);
  if (!TW) return refuse("key size not supported by the fixed-base kernels");
  pl.sb = c->crt_sb;
  pl.grp = pl.sb == GRP_TPI * L;
  pl.ps = pl.grp ? 0 : fb_pair_possible(c);
  pl.shoup = pl.ps && fb_shoup_possible(c);
  pl.gpair = pl.grp && fb_gpair_possible(c);
  pl.sgp = pl.gpair && sgp_enabled();
  pl.S = pl.ps ? pl.ps : FBGP_S;
  pl.row_words = fb_table_row_words(c);
  if (!c->fb_W) c->fb_W = fb_default_window();
  const uint64_t budget = fb_budget(c);
  pl.W = fb_choose(c, budget, &pl.sgs, allow_sgs);
  pl.K = pl.W ? fb_digit_count(c, pl.W) : 0;
  // Shoup rows: an uneven cut within the same budget where it saves a whole row product (fb_cut.hpp). K stays >= S.
  // The 4096-bit samplers and the test build's Montgomery rows keep the uniform cut.
  if (pl.shoup && pl.W) {
    const FbCut cut = fb_cut_plan(fb_exponent_bits(c), pl.W, c->fb_W, 4ull * pl.row_words, budget, pl.ps);
    pl.W = cut.W, pl.K = cut.K, pl.nw = cut.nw;
    if (pl.K < pl.ps) return refuse("fewer digit positions than limbs");
  }
  pl.raw_bits = fb_exponent_bits(c) + 64;
  const size_t sq_bits = std::max(mul(c->fb_p, c->fb_p).bits(), mul(c->fb_q, c->fb_q).bits());
  if (!pl.grp && (sq_bits > (size_t)32 * TW || c->ct_words != 2 * TW))
    return refuse("unbalanced primes: p^2 or q^2 exceeds the table row");
  if (!pl.W) return refuse("tables do not fit the device memory budget");
  if ((pl.raw_bits + 31) / 32 > FB_RAW_MAX - 2) return refuse("exponent too wide");
  // the Garner kernels take w_q < q^2 as an operand mod p^2 (k_fbg_garner: w_p + 8 p^2 - w_q > 0; k_fbp_fin: A_q, B_q <
  // 2p): keys with q >= 2p encrypt on the generic CRT path
  if (cmp(c->fb_q, shl1(c->fb_p)) >= 0) return refuse("q >= 2p: fixed-base Garner bounds");
  // the test build also keeps the samplers the product's replaced: Montgomery rows on pairs (k_fbp, $FLEXPAI_FBS=0) and
  // pair groups without the split-pair constants (k_fbgp, $FLEXPAI_SGP=0)
  if (!pl.grp && !(FLEXPAI_XCHECK ? pl.ps != 0 : pl.shoup)) return refuse("key outside the pair sampler's bounds");
  if (pl.grp && !(FLEXPAI_XCHECK ? pl.gpair : pl.sgp))
    return refuse(FLEXPAI_XCHECK ? "key outside the pair-group sampler's bounds" : "key outside the split-pair sampler's bounds");
  return pl;
}

// A build in flight: what ensure_fb's steps hand to each other. The scratch goes with it, however the build ends.
struct FbHalfConst {
  uint32_t g = 0;                                    // generator of Z_p_h*
  std::vector<uint32_t> bases;                       // [K][2][2S] pairs of B_k R and B_k^(2^LO) R mod p_h^2, R = 2^(28 S)
  std::vector<uint32_t> p, one, nm, pbig;            // p_h; pair of R mod p_h^2; c0 folding: the other prime's chunk
                                                     //   weights 2^(CB c) mod p_h and the offset 2^PB p_h
  std::vector<uint32_t> nmr, kap, fcst;              // pairs: nm R; pair of kappa R (p half); Shoup rows: mu, R^2 mod p_h
  std::vector<uint32_t> x, p2, pr2;                  // pair groups: (1 - R) mod p_h; p_h^2; p_h R' mod p_h^2 (148 limbs)
  FbRed red;                                         // exponent reduction mod p_h - 1
};
struct FbBuild {
  FbPlan pl;
  HBig primes[2], sq[2], coef;                       // p, q; p^2, q^2; (q^2)^-1 mod p^2
  FbHalfConst hc[2];
  RowScratch sc[2];
  void* t[2] = {nullptr, nullptr};                   // the tables (owned by FbTables::tables)
  uint4* sgs_rows[2] = {nullptr, nullptr};           // the 4096-bit Shoup rows' reservation (likewise)
  FbpHalf pv[2];
  FbgpHalf gv[2];
  SgpHalf sv[2];
};

// The 4096-bit Shoup rows' memory is taken before anything is built: without room for it the tables are built at the
// factored rows' own (higher) window instead of at the one chosen for both
static bool sgs_reserve(pai_ctx* c, FbBuild& b) {
  for (uint4*& r : b.sgs_rows) {
    if (!(r = (uint4*)TableArena::get().alloc(c->device, b.pl.rows() * SGS_ROW_Q * sizeof(uint4)))) return false;
    c->fb.tables.push_back(r);
  }
  return true;
}
static void sgs_unreserve(pai_ctx* c, FbBuild& b) {
  std::vector<void*>& tb = c->fb.tables;
  for (uint4*& r : b.sgs_rows) {
    if (r) tb.erase(std::find(tb.begin(), tb.end(), (void*)r)), TableArena::get().free(r);
    r = nullptr;
  }
}

// The per-half host work that needs no device -- the generator search, G = g^n mod p_h^2 (ONE powm) and the digit bases
// B_k by squarings, in the form the resident sampler's build takes -- for both halves at once on two threads (a fresh
// key's setup, HE_SA_FT re-keys per exchange)
static void fb_host_bases(const pai_ctx* c, FbBuild& b) {
  SetupTrace tr_hp("  host prep (generator, G, B_k; both halves)");
  auto prep = [&](int h) {
    FbHalfConst& o = b.hc[h];
    const HBig &P = b.primes[h], &m2 = b.sq[h];
    o.g = c->fb_g[h] ? c->fb_g[h] : fb_base(P);
    if (!o.g) return;
    HMont M2(m2);
    const int S = b.pl.S;
    const size_t RS = (size_t)LB * S;
    HBig y = M2.to(M2.pow(HBig(o.g), c->n));
    for (int k = 0; k < b.pl.K; ++k) {   // B_k = G^(2^off_k), off_k the bit offset of digit k
      const int w = fb_cut_width(k, b.pl.W, b.pl.nw);
      append(o.bases, pair_split(mul_pow2_mod(M2.from(y), RS, m2), P, S));
      append(o.bases, pair_split(mul_pow2_mod(M2.from(M2.sqr_k(y, (size_t)(w / 2))), RS, m2), P, S));
      y = M2.sqr_k(y, (size_t)w);
    }
  };
  std::thread t1(prep, 1);
  prep(0);
  t1.join();
}

// One half's remaining constants; returns the reason if the key cannot take the sampler
static const char* fb_half_consts(FbBuild& b, int h) {
  SetupTrace tr_h("  host prep (one half)");
  const FbPlan& pl = b.pl;
  FbHalfConst& o = b.hc[h];
  const HBig &P = b.primes[h], &m2 = b.sq[h];
  const HBig other = mod(b.primes[1 - h], P);
  const int S = pl.S;
  const size_t RS = (size_t)LB * S;
  o.p = P.limbs(S, LB);
  o.one = pair_split(mul_pow2_mod(HBig(1), RS, m2), P, S);
  // c0 = 1 + n M: |M| in NC chunks of CB bits; negative M through the offset 2^PB p_h
  const int CB = pl.ps ? FBP_CB : 16, NC = pl.ps ? FBP_NC : 4, PB = pl.ps ? FBP_PB : 20;
  for (int k = 0; k < NC; ++k) {
    append(o.nm, mul_pow2_mod(other, (size_t)CB * k, P).limbs(S, LB));
    if (pl.ps) append(o.nmr, mul_pow2_mod(other, (size_t)CB * k + RS, P).limbs(S, LB));   // k_fbs: gamma R joins the b sum
  }
  o.pbig = mul(P, pow2(PB)).limbs(S, LB);
  if (pl.ps) {
    // position 0's lo entries are multiplied by kappa R (FbpHalf::kapR): kappa = q^-2 mod p^2 for the p half, so that
    // the sampler leaves w_p q^-2 for k_fbp_fin; 1 (the pair of R) for the q half
    if (h == 0) o.kap = pair_split(mul_pow2_mod(b.coef, RS, m2), P, S);
    if (pl.shoup) {   // k_fbs_fill: mu = floor(R^2 / p_h) (S + 2 limbs), R^2 mod p_h (S limbs)
      const HBig R2 = pow2(2 * RS);
      const HBig mu = div_big(R2, P);
      if (mu.bits() > (size_t)LB * (S + 1)) return "Shoup rows: mu exceeds S + 1 limbs";
      o.fcst = mu.limbs(S + 2, LB);
      append(o.fcst, mod(R2, P).limbs(S, LB));
    }
  } else {
    o.x = mod(sub(add(P, HBig(1)), mul_pow2_mod(HBig(1), RS, P)), P).limbs(S, LB);
    o.p2 = m2.limbs(pl.sb, LB);
    o.pr2 = mul_pow2_mod(P, (size_t)LB * pl.sb, m2).limbs(pl.sb, LB);
  }
  const HBig D = sub(P, HBig(1));
  const std::vector<uint32_t> dw = D.words((D.bits() + 31) / 32), muw = div_big(pow2((size_t)pl.raw_bits), D).words(4);
  std::memset(&o.red, 0, sizeof(o.red));
  std::copy(dw.begin(), dw.end(), o.red.D);
  std::copy(muw.begin(), muw.end(), o.red.mu);
  o.red.dwords = (int)dw.size();
  o.red.kbits = (int)D.bits();
  return nullptr;
}

// The device side of both halves: the table, the build scratch and the constants of each, then what both share -- the
// exponent reduction and, on the 4096-bit layout that reads them, the p^2-Garner constants
static int fb_upload_halves(pai_ctx* c, FbBuild& b) {
  const FbPlan& pl = b.pl;
  FbTables& fb = c->fb;
  int rc;
  for (int h = 0; h < 2; ++h) {
    const FbHalfConst& o = b.hc[h];
    RowScratch& sc = b.sc[h];
    if (!sc.alloc(pl.K, fb_cut_width(0, pl.W, pl.nw), pl.S)) return fail(PAI_ERR_HIP, "table allocation failed");   // the widest digit's
    {
      SetupTrace tr_m("  table allocation (one half)");
      if (!(b.t[h] = TableArena::get().alloc(c->device, pl.rows() * (pl.row_words / 4) * sizeof(uint4))))
        return fail(PAI_ERR_HIP, "table allocation failed");
    }
    fb.tables.push_back(b.t[h]);
    uint32_t *p, *one, *bases, *nm, *pbig;
    if ((rc = upload_to(fb.mem, o.p, &p)) || (rc = upload_to(fb.mem, o.one, &one)) || (rc = upload_to(fb.mem, o.bases, &bases)) ||
        (rc = upload_to(fb.mem, o.nm, &nm)) || (rc = upload_to(fb.mem, o.pbig, &pbig)))
      return rc;
    const uint32_t mprime = mont_prime(b.primes[h], LB);
    if (pl.ps) {
      uint32_t *nmr, *kap = one;
      if ((rc = upload_to(fb.mem, o.nmr, &nmr)) || (h == 0 && (rc = upload_to(fb.mem, o.kap, &kap)))) return rc;
      b.pv[h] = FbpHalf{(const uint4*)b.t[h], p, one, bases, sc.lohi, nm, pbig, mprime, sc.inv, sc.pre, sc.cval, kap, nmr};
    } else {
      uint32_t *x, *p2, *pr2;
      if ((rc = upload_to(fb.mem, o.x, &x)) || (rc = upload_to(fb.mem, o.p2, &p2)) || (rc = upload_to(fb.mem, o.pr2, &pr2)))
        return rc;
      b.gv[h] = FbgpHalf{(const uint32_t*)b.t[h], p, x, one, bases, sc.lohi, nm, pbig, p2, pr2, mprime,
                         mont_prime(b.sq[h], LB), sc.inv, sc.pre, sc.cval};
      if (pl.sgp && (rc = sgp_make_half(b.primes[h], b.primes[1 - h], pl.K, b.t[h], fb.mem, &b.sv[h]))) return rc;
    }
  }
  if ((rc = upload_to(fb.mem, std::vector<FbRed>{b.hc[0].red, b.hc[1].red}, &fb.d_red))) return rc;
  if (pl.grp) {   // k_fbg_garner: p^2, 8 p^2, (q^2)^-1 R mod p^2; k_fbg_fin: q^2 R mod n^2
    const size_t RB = (size_t)LB * pl.sb, RE = (size_t)LB * c->S_e;
    fb.d_m0 = b.gv[0].p2;
    fb.mprime0 = b.gv[0].mprime2;
    if ((rc = upload_to(fb.mem, mul(b.sq[0], HBig(8)).limbs(pl.sb, LB), &fb.d_m8)) ||
        (rc = upload_to(fb.mem, mul_pow2_mod(b.coef, RB, b.sq[0]).limbs(pl.sb, LB), &fb.d_coefR)) ||
        (rc = upload_to(fb.mem, mul_pow2_mod(b.sq[1], RE, c->N).limbs(c->S_e, LB), &fb.d_q2Rn)))
      return rc;
  }
  return 0;
}

// k_fbp_fin's constants (kernels_fbp.hpp): (q^-1 R)^, (q^-2 R)^ as pairs over p, then q, q^2, p q^2, 2p, 3p
static int fbp_fin_consts(const FbBuild& b, std::vector<uint32_t>& cs) {
  const HBig &P = b.primes[0], &Q = b.primes[1], &p2 = b.sq[0];
  const int ps = b.pl.ps;
  const size_t RS = (size_t)LB * ps;
  const HBig qinv = inv_mod(mod(Q, p2), p2);
  if (qinv.is_zero()) return fail(PAI_ERR_KEY, "q not invertible mod p^2");
  cs = pair_split(mul_pow2_mod(qinv, RS, p2), P, ps);
  append(cs, pair_split(mul_pow2_mod(b.coef, RS, p2), P, ps));
  append(cs, Q.limbs(ps, LB));
  append(cs, b.sq[1].limbs(2 * ps, LB));
  append(cs, mul(P, b.sq[1]).limbs(3 * ps, LB));
  append(cs, mul(P, HBig(2)).limbs(ps, LB));
  append(cs, mul(P, HBig(3)).limbs(ps, LB));
  return 0;
}

// What the sampler and its Garner kernels read of both halves at once
static int fb_upload_sampler(pai_ctx* c, FbBuild& b) {
  const FbPlan& pl = b.pl;
  FbTables& fb = c->fb;
  int rc;
  if (pl.ps) {
    if ((rc = upload_to(fb.mem, std::vector<FbpHalf>(b.pv, b.pv + 2), &fb.d_fbp))) return rc;
    if (pl.shoup) {
      FbsConst fc[2];
      for (int h = 0; h < 2; ++h) {
        uint32_t* d;
        if ((rc = upload_to(fb.mem, b.hc[h].fcst, &d))) return rc;
        fc[h] = FbsConst{d, d + pl.ps + 2};
      }
      if ((rc = upload_to(fb.mem, std::vector<FbsConst>(fc, fc + 2), &fb.d_fbs_cst))) return rc;
    }
    std::vector<uint32_t> cs;
    if ((rc = fbp_fin_consts(b, cs)) || (rc = upload_to(fb.mem, cs, &fb.d_fbp_fin_cs))) return rc;
    fb.d_fbp_fin_p = b.pv[0].p;
    fb.fbp_fin_mprime = b.pv[0].mprime;
  } else {
    if ((rc = upload_to(fb.mem, std::vector<FbgpHalf>(b.gv, b.gv + 2), &fb.d_fbgp))) return rc;
    if (pl.sgp) {
      if ((rc = upload_to(fb.mem, std::vector<SgpHalf>(b.sv, b.sv + 2), &fb.d_sgp))) return rc;
      fb.d_sgp_q = b.sv[1].p;
    }
  }
  trace_uploads("  fb uploads");
  return 0;
}

// The factored rows of both tables (the chain products are inverted on the host between the two phases), then the build
// scratch goes back
static int fb_build_rows(pai_ctx* c, FbBuild& b) {
  const FbPlan& pl = b.pl;
  const FbTables& fb = c->fb;
  const int K = pl.K, W = pl.W;
  auto phase1 = [&] { return pl.ps ? fbp_build_phase1(pl.ps, fb.d_fbp, K, W, pl.nw, nullptr) : fbgp_build_phase1(fb.d_fbgp, K, W, nullptr); };
  auto phase2 = [&] {
    if (!pl.ps) return fbgp_build_phase2(fb.d_fbgp, (uint32_t*)b.t[0], (uint32_t*)b.t[1], K, W, nullptr);
    if constexpr (FLEXPAI_XCHECK)   // the test build's Montgomery rows
      if (!pl.shoup) return fbp_build_phase2(pl.ps, fb.d_fbp, (uint4*)b.t[0], (uint4*)b.t[1], K, W, nullptr);
    return fbs_build_phase2(pl.ps, fb.d_fbp, fb.d_fbs_cst, (uint4*)b.t[0], (uint4*)b.t[1], K, W, pl.nw, nullptr,
                            guard_args(c, (unsigned long long)pl.rows(), 0, 0, 0));
  };
  static const char* const lab[3] = {"  phase 1 (lohi, inv_fwd) + host invert", nullptr, "  phase 2 (inv_bwd, fill) + frees"};
  int rc;
  if ((rc = build_factored_rows(lab, phase1, phase2, b.primes, b.sc, 2, K, pl.S)) || (rc = guard_collect(c, nullptr))) return rc;
  SetupTrace tr_f("  scratch frees");
  for (RowScratch& s : b.sc) s.free();
  return 0;
}

// Builds everything the fixed-base path needs for window c->fb_W (or the largest smaller window within
// the memory budget). Returns 1 when the path is ready, 0 when it is unavailable (reason in fb_reason);
// never fails the caller.
static int ensure_fb(pai_ctx* c) {
  if (c->fb_state == pai_ctx::FB_READY) return 1;
  if (c->fb_state == pai_ctx::FB_UNAVAILABLE) return 0;
  FbBuild b;
  FbPlan& pl = b.pl;
  pl = fb_plan(c);
  if (pl.why) return fb_unavailable(c, pl.why);
  if (pl.sgs && !sgs_reserve(c, b)) {
    sgs_unreserve(c, b);
    pl = fb_plan(c, false);
    if (pl.why) return fb_unavailable(c, pl.why);
    if (setup_trace_on()) fprintf(stderr, "flexpai-trace Shoup rows: no room; factored rows at W = %d\n", pl.W);
  }
  SetupTrace tr_all("ensure_fb");
  const auto t0 = std::chrono::steady_clock::now();
  b.primes[0] = c->fb_p;
  b.primes[1] = c->fb_q;
  for (int h = 0; h < 2; ++h) b.sq[h] = mul(b.primes[h], b.primes[h]);
  b.coef = inv_mod(b.sq[1], b.sq[0]);
  if (b.coef.is_zero()) return fb_unavailable(c, "q^2 not invertible mod p^2");
  fb_host_bases(c, b);
  for (int h = 0; h < 2; ++h) {
    if (!(c->fb_g[h] = b.hc[h].g)) return fb_unavailable(c, "no base found");
    if (const char* why = fb_half_consts(b, h)) return fb_unavailable(c, why);
  }
  if (fb_upload_halves(c, b)) return fb_unavailable(c, pai_last_error());
  const auto t1 = std::chrono::steady_clock::now();   // fb_host_ms | fb_dev_ms
  if (fb_upload_sampler(c, b) || fb_build_rows(c, b)) return fb_unavailable(c, pai_last_error());
  if (pl.sgs) {
    SetupTrace tr_s("  Shoup rows (k_sgs_conv)");
    if (sgs_build(c, b.primes, pl.K, pl.W, b.t, b.sv, b.sgs_rows)) {
      // the factored rows are complete: k_sgp runs on them (split_sampler bit 3 stays clear)
      if (setup_trace_on()) fprintf(stderr, "flexpai-trace Shoup rows failed (%s): k_sgp at W = %d\n", pai_last_error(), pl.W);
      sgs_unreserve(c, b);
    }
  }
  const auto t2 = std::chrono::steady_clock::now();
  FbTables& fb = c->fb;
  fb.host_ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
  fb.dev_ms = std::chrono::duration<float, std::milli>(t2 - t1).count();
  fb.table_bytes = 2ull * pl.rows() * (4ull * pl.row_words + (fb.d_sgs ? 16ull * SGS_ROW_Q : 0ull));
  fb.K = pl.K;
  fb.W_used = pl.W;
  fb.nw = pl.nw;
  fb.raw_bits = pl.raw_bits;
  fb.pair_s = pl.ps;
  fb.shoup = pl.shoup;
  fb.gpair = pl.gpair;
  c->fb_state = pai_ctx::FB_READY;
  return 1;
}

// 4096-bit keys (p^2 of 148 limbs): no lane CRT; the fixed-base sampler runs on the group engine
// (kernels_grp.hpp) and k_crt_fin<8> recombines, so only its constants are set up here. Without resident
// tables, encryption takes the public-key path.
static int setup_fbg(pai_ctx* c, const HBig& p, const HBig& q) {
  constexpr int SBG = GRP_TPI * L;
  const size_t pb = std::max(p.bits(), q.bits());
  if ((size_t)LB * SBG < 2 * pb + 4 || c->tpi_e != 8) return 0;
  const size_t RE = (size_t)LB * c->S_e;
  int rc;
  if ((rc = upload(c, mul_pow2_mod(mul(q, q), 2 * RE, c->N).limbs(c->S_e, LB), &c->d_kq)) ||
      (rc = upload(c, mul_pow2_mod(mul(p, p), 2 * RE, c->N).limbs(c->S_e, LB), &c->d_kp)))
    return rc;
  c->crt_sa = 0;
  c->crt_sb = SBG;
  c->fb_p = p;
  c->fb_q = q;
  c->fbg_ok = true;
  // split-pair decryption (kernels_dec4.hpp): p_h of at most 28 * 74 - 24 bits (R >= 2^24 p_h), the ciphertext
  // in at most 4 chunks of 74 limbs; $FLEXPAI_PAIR=0 keeps the group engine's k_decrypt
  bool pair = true;
  if (const char* e = xcheck_env("FLEXPAI_PAIR")) pair = atoi(e) != 0;
  const size_t RS = (size_t)LB * D4_S;
  const int kp = (int)((32 * (size_t)c->ct_words + RS - 1) / RS);
  if (pair && pb + 24 <= RS && kp <= 4 && c->tpi_d == 4) {
    const HBig primes[2] = {p, q};
    Dec4Half dh[2];
    for (int h = 0; h < 2; ++h) {
      const HBig& ph = primes[h];
      const HBig m2 = mul(ph, ph);
      auto one_minus = [&](const HBig& r) {   // (1 - r) mod p_h for 0 < r < p_h
        return mod(sub(add(ph, HBig(1)), r), ph);
      };
      std::vector<uint32_t> pd, kf;
      if (!build_dec4f_program(ph, RS, pd, kf)) return 0;
      HBig oi = inv_mod(mod(primes[1 - h], ph), ph);
      if (oi.is_zero()) return 0;
      const HBig hh = sub(ph, oi);
      uint32_t *dp, *dx1, *dxk, *dck, *dhr, *dprog, *dkf;
      if ((rc = upload(c, ph.limbs(D4_S, LB), &dp)) ||
          (rc = upload(c, one_minus(mul_pow2_mod(HBig(1), RS, ph)).limbs(D4_S, LB), &dx1)) ||
          (rc = upload(c, one_minus(mul_pow2_mod(HBig(1), RS * kp, ph)).limbs(D4_S, LB), &dxk)) ||
          (rc = upload(c, pair_split(mul_pow2_mod(HBig(1), RS * (kp + 1), m2), ph, D4_S), &dck)) ||
          (rc = upload(c, mul_pow2_mod(hh, RS, ph).limbs(D4_S, LB), &dhr)) || (rc = upload(c, pd, &dprog)) ||
          (rc = upload(c, kf, &dkf)))
        return rc;
      dh[h] = Dec4Half{dp, dx1, dxk, dck, dhr, dprog, (int)pd.size(), mont_prime(ph, LB), dkf};
    }
    std::vector<Dec4Half> dv(dh, dh + 2);
    if ((rc = upload(c, dv, &c->d_dec4_halves))) return rc;
    c->dec4_kchunks = kp;
    c->dec4_ok = true;
  }
  return 0;
}

// A 4096-bit key's constants for the row kernels (kernels_crtw.hpp; the lane CRT kernels stop at 2048 bits): per
// half, stage A over the 74 limbs of p_h (R^(K+1) mod p_h, the op list over q_h mod (p_h - 1)), stage B over the 148
// limbs of p_h^2 (R^2, coef, the op list over p_h) and decryption (R^(K+1) mod p_h^2, the op list over p_h - 1); the
// finish reuses setup_fbg's q^2 R^2 / p^2 R^2 mod n^2 and the k_dec4 halves. Soft: an unusable key leaves rows_sa = 0.
static int setup_rows4096(pai_ctx* c, const HBig& p, const HBig& q) {
  constexpr int SA = 74, SB = 148;
  c->rows_sa = 0;
  if (c->tpi_e != 8 || !c->d_kq || std::max(p.bits(), q.bits()) + 2 > (size_t)LB * SA) return 0;
  const size_t RA = (size_t)LB * SA, RB = (size_t)LB * SB;
  const int kd = (int)((32 * (size_t)c->ct_words + RB - 1) / RB);
  if (kd > KMAX_CHUNKS) return 0;
  SetupTrace tr("    rows 4096 consts");
  const HBig primes[2] = {p, q};
  const HBig sq[2] = {mul(p, p), mul(q, q)};
  CrtHalf ha[2], hb[2], hd[2];
  int rc;
  for (int h = 0; h < 2; ++h) {
    const HBig& ph = primes[h];
    const HBig& m2 = sq[h];
    std::vector<uint32_t> pa, pb, pd;
    if (!build_lane_program(stage_a_exponent(primes[1 - h], ph), pa) || !build_lane_program(ph, pb) ||
        !build_lane_program(sub(ph, HBig(1)), pd))
      return 0;
    const HBig coef = inv_mod(sq[1 - h], m2);
    if (coef.is_zero()) return 0;
    std::vector<uint32_t> ck;
    for (int K = 1; K <= KMAX_CHUNKS; ++K) {
      std::vector<uint32_t> v = mul_pow2_mod(HBig(1), RA * (K + 1), ph).limbs(SA, LB);
      ck.insert(ck.end(), v.begin(), v.end());
    }
    std::vector<uint32_t> oneA(SA, 0), oneB(SB, 0);
    oneA[0] = oneB[0] = 1;
    uint32_t *dm, *dck, *done, *dpa, *dm2, *dr2, *dcoef, *dpb, *dck2, *done2, *dpd;
    if ((rc = upload(c, ph.limbs(SA, LB), &dm)) || (rc = upload(c, ck, &dck)) || (rc = upload(c, oneA, &done)) ||
        (rc = upload(c, pa, &dpa)) || (rc = upload(c, m2.limbs(SB, LB), &dm2)) ||
        (rc = upload(c, mul_pow2_mod(HBig(1), 2 * RB, m2).limbs(SB, LB), &dr2)) ||
        (rc = upload(c, coef.limbs(SB, LB), &dcoef)) || (rc = upload(c, pb, &dpb)) ||
        (rc = upload(c, mul_pow2_mod(HBig(1), RB * (kd + 1), m2).limbs(SB, LB), &dck2)) ||
        (rc = upload(c, oneB, &done2)) || (rc = upload(c, pd, &dpd)))
      return rc;
    ha[h] = CrtHalf{dm, dck, done, dpa, (int)pa.size(), mont_prime(ph, LB)};
    hb[h] = CrtHalf{dm2, dr2, dcoef, dpb, (int)pb.size(), mont_prime(m2, LB)};
    hd[h] = CrtHalf{dm2, dck2, done2, dpd, (int)pd.size(), mont_prime(m2, LB)};
  }
  std::vector<CrtHalf> va(ha, ha + 2), vb(hb, hb + 2), vd(hd, hd + 2);
  if ((rc = upload(c, va, &c->d_crt_a)) || (rc = upload(c, vb, &c->d_crt_b)) || (rc = upload(c, vd, &c->d_decw)))
    return rc;
  c->decw_kchunks = kd;
  c->rows_sa = SA;
  return 0;
}

// The split-pair CRT encryption of a 2049..4096-bit key holder above the rows (kernels_crt4.hpp). Stage A runs on
// setup_rows4096's stage-A halves (p_h, R^(K+1) mod p_h, the op list over q_h mod (p_h - 1)); stage B's halves are
// set up here: p_h, (1 - R) mod p_h, the plain pair of the CRT coefficient, the op list over p_h. Same gates as the
// split-pair decryption (R >= 2^24 p_h). The test build keeps its contexts -- the cross-checks' references -- on
// k_encrypt<8>. Soft: an unusable key leaves crt4_ok = false.
static int setup_crt4(pai_ctx* c, const HBig& p, const HBig& q) {
  c->crt4_ok = false;
#if FLEXPAI_XCHECK
  return 0;
#endif
  const size_t RS = (size_t)LB * D4_S;
  if (!c->fbg_ok || c->rows_sa != D4_S || !c->d_crt_a || c->tpi_e != 8 || std::max(p.bits(), q.bits()) + 24 > RS) return 0;
  SetupTrace tr("    crt4 consts");
  const HBig primes[2] = {p, q};
  const HBig sq[2] = {mul(p, p), mul(q, q)};
  Crt4Half hb[2];
  int rc;
  for (int h = 0; h < 2; ++h) {
    const HBig& ph = primes[h];
    std::vector<uint32_t> pb;
    if (!build_lane_program(ph, pb)) return 0;
    const HBig coef = inv_mod(sq[1 - h], sq[h]);
    if (coef.is_zero()) return 0;
    const HBig cb = div_big(coef, ph), ca = sub(coef, mul(cb, ph));
    std::vector<uint32_t> cpair = ca.limbs(D4_S, LB), b = cb.limbs(D4_S, LB);
    cpair.insert(cpair.end(), b.begin(), b.end());
    const HBig x1 = mod(sub(add(ph, HBig(1)), mul_pow2_mod(HBig(1), RS, ph)), ph);   // (1 - R) mod p_h
    uint32_t *dp, *dx1, *dcf, *dprog;
    if ((rc = upload(c, ph.limbs(D4_S, LB), &dp)) || (rc = upload(c, x1.limbs(D4_S, LB), &dx1)) ||
        (rc = upload(c, cpair, &dcf)) || (rc = upload(c, pb, &dprog)))
      return rc;
    hb[h] = Crt4Half{dp, dx1, dcf, dprog, (int)pb.size(), mont_prime(ph, LB)};
  }
  std::vector<Crt4Half> hv(hb, hb + 2);
  if ((rc = upload(c, hv, &c->d_crt4_b))) return rc;
  c->crt4_ok = true;
  return 0;
}

// CRT encryption constants (kernels_crt.hpp). p < q here (sorted like keypair.py:57-62).
static int setup_crt(pai_ctx* c, const HBig& p, const HBig& q) {
  c->crt_ok = c->fbg_ok = c->dec_pair_ok = c->crt_pair_ok = c->dec4_ok = c->crt4_ok = false;
  const size_t pb = std::max(p.bits(), q.bits());
  int sa = 0, sb = 0;
  for (auto cand : {std::pair<int, int>{19, 37}, std::pair<int, int>{37, 74}}) {
    if ((size_t)LB * cand.first >= pb + 2 && (size_t)LB * cand.second >= 2 * pb + 2) {
      sa = cand.first;
      sb = cand.second;
      break;
    }
  }
  if (!sa) {   // too large for the lane engine: fixed-base on the group engine, protocol-sized calls on rows
    int rc0 = setup_fbg(c, p, q);
    if (!rc0) rc0 = setup_rows4096(c, p, q);
    return rc0 ? rc0 : setup_crt4(c, p, q);
  }
  const size_t RA = (size_t)LB * sa, RB = (size_t)LB * sb, RE = (size_t)LB * c->S_e;
  const HBig primes[2] = {p, q};
  const HBig sq[2] = {mul(p, p), mul(q, q)};
  CrtHalf ha[2], hb[2], hd[2];
  int rc;
  SetupTrace tr_ab("    crt stage A/B consts");
  for (int h = 0; h < 2; ++h) {
    const HBig& ph = primes[h];
    const HBig& other = primes[1 - h];
    // stage A: (r mod p_h)^(other mod (p_h - 1)) mod p_h
    HBig ea = stage_a_exponent(other, ph);
    std::vector<uint32_t> pa, pbp;
    if (!build_lane_program(ea, pa) || !build_lane_program(ph, pbp)) return 0;
    std::vector<uint32_t> ck;
    for (int K = 1; K <= KMAX_CHUNKS; ++K) {
      std::vector<uint32_t> v = mul_pow2_mod(HBig(1), RA * (K + 1), ph).limbs(sa, LB);
      ck.insert(ck.end(), v.begin(), v.end());
    }
    std::vector<uint32_t> one(sa, 0);
    one[0] = 1;
    uint32_t *dm, *dck, *done, *dpa;
    if ((rc = upload(c, ph.limbs(sa, LB), &dm)) || (rc = upload(c, ck, &dck)) || (rc = upload(c, one, &done)) ||
        (rc = upload(c, pa, &dpa)))
      return rc;
    ha[h] = CrtHalf{dm, dck, done, dpa, (int)pa.size(), mont_prime(ph, LB)};
    // stage B: y^(p_h) mod p_h^2, times (other^2)^-1 mod p_h^2
    const HBig& m2 = sq[h];
    HBig coef = inv_mod(sq[1 - h], m2);
    if (coef.is_zero()) return 0;
    uint32_t *dm2, *dr2, *dcoef, *dpb;
    if ((rc = upload(c, m2.limbs(sb, LB), &dm2)) ||
        (rc = upload(c, mul_pow2_mod(HBig(1), 2 * RB, m2).limbs(sb, LB), &dr2)) ||
        (rc = upload(c, coef.limbs(sb, LB), &dcoef)) || (rc = upload(c, pbp, &dpb)))
      return rc;
    hb[h] = CrtHalf{dm2, dr2, dcoef, dpb, (int)pbp.size(), mont_prime(m2, LB)};
    // decryption on 16-lane rows (k_dec_w): c R mod p_h^2 by kd passes, then the op list over p_h - 1
    const int kd = (int)((32 * (size_t)c->ct_words + RB - 1) / RB);
    std::vector<uint32_t> pdw, oneb(sb, 0);
    oneb[0] = 1;
    if (kd <= KMAX_CHUNKS && build_lane_program(sub(ph, HBig(1)), pdw)) {
      uint32_t *dck2, *done2, *dpdw;
      if ((rc = upload(c, mul_pow2_mod(HBig(1), RB * (kd + 1), m2).limbs(sb, LB), &dck2)) || (rc = upload(c, oneb, &done2)) ||
          (rc = upload(c, pdw, &dpdw)))
        return rc;
      hd[h] = CrtHalf{dm2, dck2, done2, dpdw, (int)pdw.size(), mont_prime(m2, LB)};
      c->decw_kchunks = kd;
    } else {
      c->decw_kchunks = 0;
    }
  }
  std::vector<CrtHalf> va(ha, ha + 2), vb(hb, hb + 2), vd(hd, hd + 2);
  if ((rc = upload(c, va, &c->d_crt_a)) || (rc = upload(c, vb, &c->d_crt_b))) return rc;
  if (c->decw_kchunks && (rc = upload(c, vd, &c->d_decw))) return rc;
  // finish: q^2 R^2 mod n^2 and p^2 R^2 mod n^2 (group layout)
  if ((rc = upload(c, mul_pow2_mod(sq[1], 2 * RE, c->N).limbs(c->S_e, LB), &c->d_kq)) ||
      (rc = upload(c, mul_pow2_mod(sq[0], 2 * RE, c->N).limbs(c->S_e, LB), &c->d_kp)))
    return rc;
  c->crt_sa = sa;
  c->crt_sb = sb;
  c->crt_ok = true;
  c->fb_p = p;   // the fixed-base tables are built lazily (ensure_fb)
  c->fb_q = q;
  // lane decryption's CRT constants (p, q, q^-1 R mod p), shared by the pair kernels' k_dec_fin_pair
  {
    SetupTrace tr_d("    lane decrypt consts");
    if ((int)((32 * (size_t)c->ct_words + RB - 1) / RB) > KMAX_CHUNKS) return 0;
    HBig qinv = inv_mod(mod(q, p), p);
    if ((rc = upload(c, p.limbs(sa, LB), &c->d_dec_p)) || (rc = upload(c, q.limbs(sa, LB), &c->d_dec_q)) ||
        (rc = upload(c, mul_pow2_mod(qinv, RA, p).limbs(sa, LB), &c->d_dec_qinvR)))
      return rc;
    c->dec_pprime = mont_prime(p, LB);
    c->dec_lane_ok = true;
  }
  // pair kernels: residues mod p_h^2 as (A, B) over the sa limbs of p_h, R = 2^(28 sa) >= 2^12 p_h
  bool pair = true;
  if (const char* e = xcheck_env("FLEXPAI_PAIR")) pair = atoi(e) != 0;
  if (pair && (size_t)LB * sa >= pb + 12) {
    SetupTrace tr_p("    pair consts");
    const int S2 = 2 * sa;
    const int kp = (int)((32 * (size_t)c->ct_words + RA - 1) / RA);
    std::vector<uint32_t> one(S2, 0);
    one[0] = 1;
    DecPairHalf dp[2];
    CrtHalf pw[2], pbh[2];
    for (int h = 0; h < 2; ++h) {
      const HBig& ph = primes[h];
      const HBig& other = primes[1 - h];
      const HBig& m2 = sq[h];
      std::vector<uint32_t> pd, pe, kf;
      const bool decf = !(xcheck_env("FLEXPAI_DECF") && atoi(xcheck_env("FLEXPAI_DECF")) == 0);
      if (!(decf ? build_decf_lane_program(ph, RA, sa, pd, kf) : build_lane_program(sub(ph, HBig(1)), pd)) ||
          !build_lane_program(ph, pe))
        return 0;
      c->decf = decf;
      HBig oi = inv_mod(mod(other, ph), ph);
      HBig coef = inv_mod(sq[1 - h], m2);
      if (oi.is_zero() || coef.is_zero()) return 0;
      const uint32_t mp1 = mont_prime(ph, LB);
      uint32_t *dph, *dck, *dhR, *dpm1, *done, *dprog, *dr2, *dcoef, *dpe, *dkf = nullptr;
      if ((rc = upload(c, ph.limbs(sa, LB), &dph)) ||
          (rc = upload(c, pair_split(mul_pow2_mod(HBig(1), RA * (kp + 1), m2), ph, sa), &dck)) ||
          (rc = upload(c, mul_pow2_mod(sub(ph, oi), RA, ph).limbs(sa, LB), &dhR)) ||
          (rc = upload(c, sub(ph, HBig(1)).limbs(sa, LB), &dpm1)) || (rc = upload(c, one, &done)) ||
          (rc = upload(c, pd, &dprog)) || (rc = upload(c, pair_split(mul_pow2_mod(HBig(1), 2 * RA, m2), ph, sa), &dr2)) ||
          (rc = upload(c, pair_split(coef, ph, sa), &dcoef)) || (rc = upload(c, pe, &dpe)) ||
          (!kf.empty() && (rc = upload(c, kf, &dkf))))
        return rc;
      dp[h] = DecPairHalf{dph, dck, dhR, dpm1, mp1, 0u};
      pw[h] = CrtHalf{dph, dkf, done, dprog, (int)pd.size(), mp1};
      pbh[h] = CrtHalf{dph, dr2, dcoef, dpe, (int)pe.size(), mp1};
    }
    std::vector<DecPairHalf> dpv(dp, dp + 2);
    std::vector<CrtHalf> pwv(pw, pw + 2), pbv(pbh, pbh + 2);
    HBig maxint = sub(div_small(c->n, 3), HBig(1));
    if ((rc = upload(c, dpv, &c->d_decp_halves)) || (rc = upload(c, pwv, &c->d_decp_pow)) ||
        (rc = upload(c, pbv, &c->d_crtp_b)) || (rc = upload(c, c->n.limbs(S2, LB), &c->d_decp_nl)) ||
        (rc = upload(c, maxint.limbs(S2, LB), &c->d_decp_maxint)))
      return rc;
    c->decp_kchunks = kp;
    c->dec_pair_ok = c->dec_lane_ok;   // shares the lane decrypt's p, q, q^-1 R constants
    c->crt_pair_ok = true;
  }
  return 0;
}

static int set_private_impl(pai_ctx* c, HBig p, HBig q);
static void pool_drop(pai_ctx* c);

// Transactional: on any failure every private-key allocation of this call is released and the
// context is left exactly as before (public-key operations keep working, a retry starts clean).
// The fixed-base tables are not built here (ensure_fb, on the first device-RNG encryption).
int pai_ctx_set_private(pai_ctx* c, const uint8_t* p_le, const uint8_t* q_le, size_t half_bytes) {
  if (!c || !p_le || !q_le) return fail(PAI_ERR_ARG, "pai_ctx_set_private: null argument");
  CtxLock lk(c);
  HIPCHK(hipSetDevice(c->device));
  HBig p = HBig::from_le_bytes(p_le, half_bytes), q = HBig::from_le_bytes(q_le, half_bytes);
  if (cmp(mul(p, q), c->n) != 0) return fail(PAI_ERR_KEY, "given public key does not match the given p and q");
  if (cmp(p, q) == 0) return fail(PAI_ERR_KEY, "p and q have to be different");
  if (cmp(q, p) < 0) std::swap(p, q);   // keypair.py:57-62
  if (c->has_priv) return 0;            // same key (p q == n): already set
  pool_drop(c);                         // the pool belongs to the party the context was; a key holder fills its own
  c->in_priv = true;
  int rc;
  {
    SetupTrace tr("pai_ctx_set_private");
    rc = set_private_impl(c, p, q);
  }
  trace_uploads("  set_private uploads");
  c->in_priv = false;
  if (!rc && !c->holder) {
    c->holder = true;
    ++g_key_holders;
  }
  if (rc) {
    const std::string msg = g_last_error;
    for (void* a : c->priv_allocs) (void)hipFree(a);
    c->priv_allocs.clear();
    (void)hipGetLastError();
    c->has_priv = c->crt_ok = c->fbg_ok = c->dec_lane_ok = c->dec_pair_ok = c->crt_pair_ok = c->dec4_ok = c->crt4_ok = false;
    c->d_decw = nullptr;
    c->decw_kchunks = 0;
    c->rows_sa = 0;
    c->fb_state = pai_ctx::FB_UNTRIED;
    g_last_error = msg;
  }
  return rc;
}

static int set_private_impl(pai_ctx* c, HBig p, HBig q) {
  const int S = c->S_d;
  const size_t Rbits = (size_t)LB * S;
  HBig hp, hq;
  {
    HBig qi = inv_mod(q, p), pi = inv_mod(p, q);
    if (qi.is_zero() || pi.is_zero()) return fail(PAI_ERR_KEY, "p, q not coprime");
    hp = sub(p, qi);   // (-q)^-1 mod p == L(g^(p-1) mod p^2, p)^-1 (keypair.py:81-90, g = n + 1)
    hq = sub(q, pi);
  }
  HBig primes[2] = {p, q}, hs[2] = {hp, hq};
  size_t ebits = std::max(sub(p, HBig(1)).bits(), sub(q, HBig(1)).bits());
  c->nwin = (int)((ebits + 4) / 5);
  DecHalf hh[2];
  int rc;
  for (int h = 0; h < 2; ++h) {
    const HBig& ph = primes[h];
    HBig m = mul(ph, ph);
    HBig e = sub(ph, HBig(1));
    std::vector<uint8_t> dig(c->nwin);
    for (int w = 0; w < c->nwin; ++w) {
      int v = 0;
      for (int b = 4; b >= 0; --b) v = (v << 1) | e.bit((size_t)(c->nwin - 1 - w) * 5 + b);
      dig[w] = (uint8_t)v;
    }
    uint32_t *dm, *dR3, *done, *dpneg, *dph, *dhR;
    uint8_t* ddig;
    HBig pneg = sub(pow2(Rbits), ph);
    if ((rc = upload(c, m.limbs(S, LB), &dm)) ||
        (rc = upload(c, mul_pow2_mod(HBig(1), 3 * Rbits, m).limbs(S, LB), &dR3)) ||
        (rc = upload(c, mul_pow2_mod(HBig(1), Rbits, m).limbs(S, LB), &done)) ||
        (rc = upload(c, pneg.limbs(S, LB), &dpneg)) || (rc = upload(c, ph.limbs(S, LB), &dph)) ||
        (rc = upload(c, mul_pow2_mod(hs[h], Rbits, ph).limbs(S, LB), &dhR)) || (rc = upload(c, dig, &ddig)))
      return rc;
    hh[h] = DecHalf{dm, dR3, done, dpneg, dph, dhR, ddig, mont_prime(m, LB), mont_prime(pneg, LB), mont_prime(ph, LB), 0u};
  }
  std::vector<DecHalf> hv(hh, hh + 2);
  if ((rc = upload(c, hv, &c->d_halves))) return rc;
  HBig qinv = inv_mod(q, p);
  HBig maxint = sub(div_small(c->n, 3), HBig(1));   // keypair.py:29
  if ((rc = upload(c, mul_pow2_mod(qinv, Rbits, p).limbs(S, LB), &c->d_qinvR)) ||
      (rc = upload(c, c->n.limbs(S, LB), &c->d_nlimb)) ||
      (rc = upload(c, mul_pow2_mod(mod(q, c->n), Rbits, c->n).limbs(S, LB), &c->d_qRn)) ||
      (rc = upload(c, maxint.limbs(S, LB), &c->d_maxint)))
    return rc;
  c->nprime_d = mont_prime(c->n, LB);
  c->n_limbs = (int)((c->n.bits() + LB - 1) / LB);
  c->has_priv = true;
  SetupTrace tr("  setup_crt");
  if ((rc = setup_crt(c, p, q))) return rc;
  // a key outside the pair kernels' bounds (R = 2^(28 S) >= 2^12 p_h) -- or a test build's $FLEXPAI_PAIR=0 context --
  // encrypts on the public-key kernels and decrypts on the group engine (the 2S-limb lane kernels were retired in
  // round 6)
  if (c->crt_ok && !c->crt_pair_ok) c->crt_ok = false;
  if (c->dec_lane_ok && !c->dec_pair_ok) c->dec_lane_ok = false;
  return 0;
}

void pai_ctx_destroy(pai_ctx* c) { delete c; }

void pai_release_table_cache(void) { TableArena::get().trim(); }

int pai_ctx_set_option(pai_ctx* c, int option, int value) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  switch (option) {
    case PAI_OPT_CRT_ENCRYPT: c->crt_enabled = value != 0; return 0;
    case PAI_OPT_ROWS_MAX:
      if (value < 0) return fail(PAI_ERR_ARG, "PAI_OPT_ROWS_MAX must be >= 0");
      c->crtw_max = value;
      return 0;
    case PAI_OPT_CRT4_MIN:
      if (value < 0) return fail(PAI_ERR_ARG, "PAI_OPT_CRT4_MIN must be >= 0");
      c->crt4_min = value;
      return 0;
    case PAI_OPT_MATMUL_FUSED: c->mm_fused = value != 0; return 0;
    case PAI_OPT_SEGDOT_FUSED: c->sd_fused = value != 0; return 0;
    case PAI_OPT_POOL_FUSED: c->pool.fused = value != 0; return 0;
    case PAI_OPT_SCAN_TILE:
      if (value < 0) return fail(PAI_ERR_ARG, "PAI_OPT_SCAN_TILE must be >= 0");
      c->scan_tile = value;
      return 0;
    case PAI_OPT_FOLD_ROWS:
      if (value < 0 || value > 2) return fail(PAI_ERR_ARG, "PAI_OPT_FOLD_ROWS must be 0, 1 or 2");
      c->fold_rows = value;
      return 0;
    case PAI_OPT_OBF_CHUNK:
      if (value < 64) return fail(PAI_ERR_ARG, "PAI_OPT_OBF_CHUNK must be >= 64");
      c->obf_chunk = value;
      return 0;
    case PAI_OPT_STAGE_TIMING: c->timing = value != 0; stage_reset(c); return 0;
    case PAI_OPT_LANE_DECRYPT: c->dec_lane_enabled = value != 0; return 0;
    case PAI_OPT_FIXED_BASE: c->fb_enabled = value != 0; return 0;
    case PAI_OPT_PUBLIC_FB: c->pfb_enabled = value != 0; return 0;
    case PAI_OPT_PFB_WINDOW:
      if (!pfb_window_ok(value)) return fail(PAI_ERR_ARG, "public fixed-base window must be 12, 16 or 20");
      if (value == c->pfb_W) return 0;
      c->pfb_W = value;
      HIPCHK(hipSetDevice(c->device));
      c->pfb.release();
      c->pfb_state = pai_ctx::FB_UNTRIED;
      return 0;
    case PAI_OPT_FB_WINDOW:
      if (!fb_window_ok(value)) return fail(PAI_ERR_ARG, "fixed-base window must be 8, 12, 16 or 20 .. 24");
      if (value == c->fb_W) return 0;
      c->fb_W = value;
      HIPCHK(hipSetDevice(c->device));
      c->fb.release();                       // rebuilt lazily for the new window
      c->fb_state = pai_ctx::FB_UNTRIED;
      return 0;
  }
  return fail(PAI_ERR_ARG, "pai_ctx_set_option: unknown option");
}

int pai_ctx_get_option(const pai_ctx* c, int option, int* value) {
  if (!c || !value) return fail(PAI_ERR_ARG, "null argument");
  CtxLock lk(c);
  switch (option) {
    case PAI_OPT_CRT_ENCRYPT: *value = c->crt_enabled ? 1 : 0; return 0;
    case PAI_OPT_CRT_AVAILABLE: *value = c->crt_ok ? 1 : 0; return 0;
    case PAI_OPT_ROWS_MAX: *value = (int)std::min<long long>(c->crtw_max, INT32_MAX); return 0;
    case PAI_OPT_CRT4_MIN: *value = (int)std::min<long long>(c->crt4_min, INT32_MAX); return 0;
    case PAI_OPT_MATMUL_FUSED: *value = c->mm_fused ? 1 : 0; return 0;
    case PAI_OPT_MATMUL_PATH: *value = c->mm_path; return 0;
    case PAI_OPT_SEGDOT_FUSED: *value = c->sd_fused ? 1 : 0; return 0;
    case PAI_OPT_SEGDOT_PATH: *value = c->sd_path; return 0;
    case PAI_OPT_POOL_FUSED: *value = c->pool.fused ? 1 : 0; return 0;
    case PAI_OPT_SCAN_TILE: *value = c->scan_tile; return 0;
    case PAI_OPT_SCAN_PATH: *value = c->scan_path; return 0;
    case PAI_OPT_FOLD_ROWS: *value = c->fold_rows; return 0;
    case PAI_OPT_FOLD_PATH: *value = c->fold_path; return 0;
    case PAI_OPT_OBF_CHUNK: *value = c->obf_chunk; return 0;
    case PAI_OPT_STAGE_TIMING: *value = c->timing ? 1 : 0; return 0;
    case PAI_OPT_LANE_DECRYPT: *value = (c->dec_lane_ok && c->dec_lane_enabled) ? 1 : 0; return 0;
    // 1 when device-RNG encryption will use the fixed bases (tables resident, or not yet tried)
    case PAI_OPT_FIXED_BASE:
      *value = ((c->crt_ok || c->fbg_ok) && c->fb_enabled && c->fb_state != pai_ctx::FB_UNAVAILABLE) ? 1 : 0;
      return 0;
    case PAI_OPT_FB_WINDOW: *value = c->fb.W_used ? c->fb.W_used : c->fb_W ? c->fb_W : fb_default_window(); return 0;
    case PAI_OPT_FB_READY: *value = c->fb_state == pai_ctx::FB_READY ? 1 : 0; return 0;
    case PAI_OPT_PUBLIC_FB:
      *value = (pfb_supported(c) && c->pfb_enabled && c->pfb_state != pai_ctx::FB_UNAVAILABLE) ? 1 : 0;
      return 0;
    case PAI_OPT_PFB_READY: *value = c->pfb_state == pai_ctx::FB_READY ? 1 : 0; return 0;
    case PAI_OPT_PFB_WINDOW: *value = c->pfb.W_used ? c->pfb.W_used : c->pfb_W ? c->pfb_W : pfb_default_window(); return 0;
    case PAI_OPT_FB_PAIR:
      *value = c->fb_state == pai_ctx::FB_READY ? (c->fb.gpair ? FBGP_S : c->fb.pair_s) : 0;
      return 0;
    case PAI_OPT_SPLIT_SAMPLER:
      *value = (c->fb_state == pai_ctx::FB_READY && c->fb.d_sgp ? 1 : 0) |
               (c->pfb_state == pai_ctx::FB_READY && c->pfb.d_sgp ? 2 : 0) |
               (c->fb_state == pai_ctx::FB_READY && c->fb.shoup ? 4 : 0) |
               (c->fb_state == pai_ctx::FB_READY && c->fb.d_sgs ? 8 : 0);
      return 0;
    case PAI_OPT_PAIR:
      *value = ((c->dec_pair_ok || c->dec4_ok) && c->dec_lane_enabled ? 1 : 0) | (c->crt_pair_ok ? 2 : 0) |
               (c->pe_ok || c->pe1_ok || (c->pe4_ok && !c->has_priv) ? 4 : 0) | (c->crt4_ok ? 8 : 0);
      return 0;
  }
  return fail(PAI_ERR_ARG, "pai_ctx_get_option: unknown option");
}

int pai_ctx_stage_times(pai_ctx* c, float* ms_out, int max_out, int* count) {
  if (!c || !count) return fail(PAI_ERR_ARG, "null argument");
  CtxLock lk(c);
  *count = 0;
  if (c->nev < 2) return 0;
  HIPCHK(hipSetDevice(c->device));
  if (c->nchunk_ev > 0) HIPCHK(hipEventSynchronize(c->ev[c->nchunk_ev - 1][c->nev - 1]));
  const int k = std::min(c->nev - 1, max_out);
  for (int i = 0; i < k; ++i) {
    ms_out[i] = 0.f;
    for (int ch = 0; ch < c->nchunk_ev; ++ch) {
      float t = 0.f;
      HIPCHK(hipEventElapsedTime(&t, c->ev[ch][i], c->ev[ch][i + 1]));
      ms_out[i] += t;
    }
  }
  *count = k;
  return 0;
}

int pai_ctx_fixed_base_info(pai_ctx* c, uint32_t* g_p, uint32_t* g_q, int* digits, int* window) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (!c->crt_ok && !c->fbg_ok)
    return fail(PAI_ERR_NOPRIV, "fixed-base obfuscation not available (needs the private key)");
  HIPCHK(hipSetDevice(c->device));
  if (!ensure_fb((pai_ctx*)c)) return fail(PAI_ERR_KEY, "fixed-base obfuscation not available: " + c->fb_reason);
  if (g_p) *g_p = c->fb_g[0];
  if (g_q) *g_q = c->fb_g[1];
  if (digits) *digits = c->fb.K;
  if (window) *window = c->fb.W_used;
  return 0;
}

int pai_ctx_fixed_base_prepare(pai_ctx* c) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (!c->crt_ok && !c->fbg_ok)
    return fail(PAI_ERR_NOPRIV, "fixed-base obfuscation not available (needs the private key)");
  HIPCHK(hipSetDevice(c->device));
  if (!ensure_fb(c)) return fail(PAI_ERR_KEY, "fixed-base obfuscation not available: " + c->fb_reason);
  return 0;
}

// The window ensure_fb would choose and its break-even element count (0 when the tables are resident or
// the path is unavailable: nothing left to decide).
static long long fb_threshold(pai_ctx* c) {
  if (c->fb_state != pai_ctx::FB_UNTRIED) return 0;
  const FbPlan pl = fb_plan(c);
  return pl.W ? fb_break_even(c, pl.rows(), 4 * pl.row_words + (pl.sgs ? 16 * SGS_ROW_Q : 0)) : 0;
}

static bool fb_wanted(pai_ctx* c, long long n) {
  if (c->fb_state != pai_ctx::FB_UNTRIED) return true;   // resident, or known unavailable (ensure_fb says)
  if (c->fb_call) return c->fb_call > 0;                 // a host-buffer call decided once for all chunks
  c->fb_seen += n;
  return c->fb_seen >= fb_threshold(c);
}

int pai_ctx_fixed_base_policy(pai_ctx* c, long long* seen, long long* threshold) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (seen) *seen = c->fb_seen;
  if (threshold) *threshold = fb_threshold(c);
  return 0;
}

int pai_ctx_fixed_base_setup(const pai_ctx* c, float* host_ms, float* device_ms, uint64_t* table_bytes) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (c->fb_state != pai_ctx::FB_READY) return fail(PAI_ERR_KEY, "fixed-base tables are not resident");
  if (host_ms) *host_ms = c->fb.host_ms;
  if (device_ms) *device_ms = c->fb.dev_ms;
  if (table_bytes) *table_bytes = c->fb.table_bytes;
  return 0;
}

int pai_ctx_info(const pai_ctx* c, int* key_bits, int* ct_words, int* pt_words) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (key_bits) *key_bits = c->nb;
  if (ct_words) *ct_words = c->ct_words;
  if (pt_words) *pt_words = c->pt_words;
  return 0;
}

// ------------------------------------------------------------------ device entry points
// The description of elements [off, ...) of the call e (kernels.hpp: plaintext source, obfuscator source, output): every
// launcher's chunk loop takes its slice here.
static int enc_r_words(const EncParams& e) {   // the words of r the kernels read (EncObf::r_words)
  return e.obf == PAI_OBF_GIVEN ? e.r_words : e.obf == PAI_OBF_RNG ? e.rng_words : 0;
}
struct EncSlice {
  EncPlain src;
  EncObf rnd;
  EncOut dst;
};
static EncSlice enc_slice(const EncParams& e, long long off) {
  EncSlice s{};
  s.src = EncPlain{(const char*)e.x + (size_t)off * (e.dtype == PAI_F32 ? 4 : 8), e.dtype, e.exp_mode, e.fexp};
  s.rnd.obf = e.obf;
  s.rnd.r = e.r ? e.r + (size_t)off * e.r_stride : nullptr;
  s.rnd.r_stride = e.r_stride;
  s.rnd.r_words = enc_r_words(e);
  std::memcpy(s.rnd.rng_key, e.rng_key, sizeof(s.rnd.rng_key));
  s.rnd.index_base = e.index_base + (unsigned long long)off;
  s.dst = EncOut{e.ct + (size_t)off * e.ct_words, e.exp + off, e.status ? e.status + off : nullptr, e.ct_words};
  return s;
}
// ... into a parameter struct that keeps the fields flat (EncParams, PeParams, Pe1Params: kernels.hpp says why)
template <class P>
static void set_flat(P& p, const EncSlice& s) {
  p.x = s.src.x;
  p.dtype = s.src.dtype;
  p.exp_mode = s.src.exp_mode;
  p.fexp = s.src.fexp;
  p.obf = s.rnd.obf;
  p.r = s.rnd.r;
  p.r_stride = s.rnd.r_stride;
  p.r_words = p.rng_words = s.rnd.r_words;
  std::memcpy(p.rng_key, s.rnd.rng_key, sizeof(p.rng_key));
  p.index_base = s.rnd.index_base;
  p.ct = s.dst.ct;
  p.exp = s.dst.exp;
  p.status = s.dst.status;
  p.ct_words = s.dst.ct_words;
}

// words of r that device RNG draws per element: 64 bits more than n
static int rng_stream_words(const pai_ctx* c) { return (c->nb + 64 + 31) / 32; }

// What encrypt_route (encrypt_route.hpp) reads of a context.
static pai_route_facts route_facts(const pai_ctx* c) {
  pai_route_facts f{};
  f.has_priv = c->has_priv;
  f.crt_enabled = c->crt_enabled;
  f.fb_enabled = c->fb_enabled;
  f.pfb_enabled = c->pfb_enabled;
  f.crt_ok = c->crt_ok;
  f.crt_sa = c->crt_sa;
  f.fbg_ok = c->fbg_ok;
  f.rows_sa = c->rows_sa;
  f.crt4_ok = c->crt4_ok;
  f.pe_ok = c->pe_ok;
  f.pe1_ok = c->pe1_ok;
  f.pe4_ok = c->pe4_ok;
  f.pew_ok = c->d_pew_prog != nullptr;
  f.pfb_supported = pfb_supported(c);
  f.ct_words = c->ct_words;
  // the rows stage r in crtw::RW_WORDS words and reduce it in at most KMAX_CHUNKS chunks of rows_sa limbs
  f.rows_r_max = std::min(crtw::RW_WORDS, KMAX_CHUNKS * LB * c->rows_sa / 32);
  f.crtw_max = c->crtw_max;
  f.crt4_min = c->crt4_min;
  return f;
}

template <int TPI>
static int launch_encrypt(pai_ctx* c, EncParams& p, hipStream_t st) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  const size_t lds = (size_t)GPB * S * 4;
  const int grid = grid_for(c, k_encrypt<TPI>, lds, p.n, GPB);
  int rc = ensure_scratch(c, (size_t)grid * BLOCK * TILE_WORDS_PER_LANE * 4);
  if (rc) return rc;
  p.scratch = (uint32_t*)c->d_scratch;
  stage_mark(c, 0, st);
  hipLaunchKernelGGL(k_encrypt<TPI>, dim3(grid), dim3(BLOCK), lds, st, p);
  HIPCHK(hipGetLastError());
  stage_mark(c, 1, st);
  return 0;
}

// CRT encryption (kernels_crt.hpp) in chunks of CRT_CHUNK elements: stage A (mod p, q), stage B
// (mod p^2, q^2), finish (mod n^2), all asynchronous on `st`.
constexpr long long CRT_CHUNK = 1ll << 22;

template <int TPI>
static int launch_crt_fin(pai_ctx* c, CrtFinParams& f, hipStream_t st) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  const size_t lds = (size_t)GPB * S * 4;
  const int grid = grid_for(c, k_crt_fin<TPI>, lds, f.n, GPB);
  hipLaunchKernelGGL(k_crt_fin<TPI>, dim3(grid), dim3(BLOCK), lds, st, f);
  HIPCHK(hipGetLastError());
  return 0;
}

// Fixed-base encryption (kernels_fb.hpp), chunks of CRT_CHUNK elements: exponent digits, the per-half
// table products with c0 folded in, Garner recombination into the ciphertext words.
static int launch_fb(pai_ctx* c, const EncParams& e, hipStream_t st) {
  const int SB = c->crt_sb;
  const bool grp = SB == GRP_TPI * L;
  const long long N = e.n;
  const long long chunk = std::min(N, CRT_CHUNK);
  const int K = c->fb.K, W = c->fb.W_used;
  int occF = 1;
#if FLEXPAI_XCHECK
  if (grp && !c->fb.gpair) return fail(PAI_ERR_KEY, "fixed-base encrypt: no pair tables");
  if (grp && !c->fb.d_sgp) fbgp_occupancy(&occF);
  if (!grp && !c->fb.pair_s) return fail(PAI_ERR_KEY, "fixed-base encrypt: no pair tables");
#else
  if (grp && !(c->fb.gpair && c->fb.d_sgp)) return fail(PAI_ERR_KEY, "fixed-base encrypt: no split-pair tables");
  if (!grp && !c->fb.shoup) return fail(PAI_ERR_KEY, "fixed-base encrypt: no Shoup tables");
#endif
#if FLEXPAI_XCHECK
  if (c->fb.pair_s && !c->fb.shoup && fbp_occupancy(c->fb.pair_s, &occF)) return fail(PAI_ERR_KEY, "fixed-base encrypt: unsupported size");
#endif
  if (c->fb.shoup && fbs_occupancy(c->fb.pair_s, &occF)) return fail(PAI_ERR_KEY, "fixed-base encrypt: unsupported size");
  // elements per block: one per lane, one per lane pair (k_fbs), or one per lane group (grp)
  const int EPB = grp ? BLOCK / GRP_TPI : c->fb.shoup ? LANE_BLOCK / 2 : LANE_BLOCK;
  const long long lane_blocks = (chunk + EPB - 1) / EPB;
  const int gxF = (int)std::max<long long>(1, std::min<long long>(lane_blocks, (long long)occF * c->cus / 2));
  const size_t dbytes = (size_t)2 * K * 4, wbytes = (size_t)2 * std::max(SB, 2 * c->fb.pair_s) * 4;   // per element
  int rc;
  const size_t sbytes = c->fb.d_sgs ? (size_t)2 * (16 * sizeof(uint4) + 2 * 4) : 0;   // k_sgs's b sums
  if ((rc = ensure_work(c, dbytes * chunk + wbytes * (size_t)fbp_npad(chunk) + sbytes * chunk))) return rc;   // pairs: 64-element tiles
  uint32_t* digits = (uint32_t*)c->d_work;
  uint32_t* w = (uint32_t*)((char*)c->d_work + dbytes * chunk);
  uint4* sgs_bsum = (uint4*)((char*)w + wbytes * (size_t)fbp_npad(chunk));
  int dbg_stage = 0;   // test build: $FLEXPAI_DEBUG_SGS_STAGE = 1 stops after k_sgs, 2 after the b sums (or k_sgp)
#if FLEXPAI_XCHECK
  if (const char* ds = getenv("FLEXPAI_DEBUG_SGS_STAGE")) dbg_stage = atoi(ds);
#endif
  uint32_t* sgs_bcc = (uint32_t*)(sgs_bsum + (size_t)2 * 16 * chunk);
  for (long long off = 0; off < N; off += chunk) {
    const long long n = std::min(chunk, N - off);
    const EncSlice sl = enc_slice(e, off);
    FbDigitParams pd{};
    pd.n = n;
    std::memcpy(pd.rng_key, sl.rnd.rng_key, sizeof(pd.rng_key));
    pd.index_base = sl.rnd.index_base;
    pd.K = K;
    pd.W = W;
    pd.nw = c->fb.nw;
    pd.raw_bits = c->fb.raw_bits;
    pd.red = c->fb.d_red;
    pd.digits = digits;
    const unsigned long long dig_words = (unsigned long long)2 * K * chunk, w_words = wbytes * (size_t)fbp_npad(chunk) / 4;
    pd.g = guard_args(c, 0, dig_words, 0, 0);
    const int gD = (int)std::min<long long>((long long)8 * c->cus, (n + FB_DIG_BLOCK - 1) / FB_DIG_BLOCK);
    stage_mark(c, 0, st);
    HIPCHK(fb_launch_digits(pd, gD, st));
    stage_mark(c, 1, st);
    const int gF = (int)std::min<long long>(gxF, (n + EPB - 1) / EPB);
    const FbgpParams pg{c->fb.d_fbgp, n, K, W, digits, w, sl.src, sl.dst};   // the test build's k_fbgp, and k_fbgp_w
    if (c->fb.pair_s) {
      FbpParams pp{c->fb.d_fbp, n, K, W, digits, w, sl.src, sl.dst};
      pp.nw = c->fb.nw;
      pp.g = guard_args(c, fb_cut_row(K, W, pp.nw), dig_words, w_words, 0);
#if FLEXPAI_XCHECK
      if (!c->fb.shoup) HIPCHK(fbp_launch(c->fb.pair_s, pp, gF, st));
#endif
      if (c->fb.shoup) HIPCHK(fbs_launch(c->fb.pair_s, pp, gF, st));
    } else if (grp && c->fb.gpair) {
      if (c->fb.d_sgs) {   // split pairs on Shoup rows (kernels_sgs.hpp), then the b sums applied
        int occS = 1;
        sgs_occupancy(&occS);
        SgsParams sp{c->fb.d_sgs, n, K, W, digits, w, sgs_bsum, sgs_bcc};
        sp.g = guard_args(c, (unsigned long long)K << W, dig_words, w_words, 0);
        const long long nb = (n + SGP_PAIRS - 1) / SGP_PAIRS;
        HIPCHK(sgs_launch(sp, (int)std::max<long long>(1, std::min<long long>(nb, (long long)occS * c->cus / 2)), 2, st));
        const SgsFinParams sf{c->fb.d_sgs, n, w, sgs_bsum, sgs_bcc, sl.src, sl.dst.exp, sl.dst.status, dbg_stage};
        if (dbg_stage != 1) HIPCHK(sgs_launch_bfin(sf, 2, c->cus, st));
      } else if (c->fb.d_sgp) {   // split pairs (kernels_sgp.hpp): SGP_PAIRS elements per block, grid (gx, 2)
        int occS = 1;
        sgp_occupancy(&occS);
        SgpParams sp{c->fb.d_sgp, n, K, W, digits, w, sl.src, sl.dst};
        sp.g = guard_args(c, (unsigned long long)K << W, dig_words, w_words, 0);
        const long long nb = (n + SGP_PAIRS - 1) / SGP_PAIRS;
        HIPCHK(sgp_launch(sp, (int)std::max<long long>(1, std::min<long long>(nb, (long long)occS * c->cus / 2)), 2, st));
      } else {
#if FLEXPAI_XCHECK
        HIPCHK(fbgp_launch(pg, gF, st));
#endif
      }
    }
    stage_mark(c, 2, st);
    c->fb_last_w = w;
    c->fb_last_n = n;
    if (dbg_stage) continue;
    if (grp) {   // w_h = c0 G_h^(a_h) mod p_h^2 -> Garner: h mod p^2 (S = 148), c = w_q + q^2 h mod n^2 (S = 296)
      int occH = 1, occC = 1;
      grp_fin_occupancy(&occH, &occC);
      if (c->fb.gpair && c->fb.d_sgp) {   // the pairs -> w_h = A + p_h B mod p_h^2 (timed with the fin stage)
        SgpParams sw{};
        sw.halves = c->fb.d_sgp;
        sw.n = n;
        sw.out = w;
        HIPCHK(sgp_launch_w(sw, 2, c->cus, st));
      } else if (c->fb.gpair) {
        const long long gb4 = (n + BLOCK / 4 - 1) / (BLOCK / 4);
        HIPCHK(fbgp_launch_w(pg, (int)std::max<long long>(1, std::min<long long>(gb4, (long long)occH * c->cus / 2)), st));
      }
      const long long gb4 = (n + BLOCK / GRP_TPI - 1) / (BLOCK / GRP_TPI), gb8 = (n + BLOCK / 8 - 1) / (BLOCK / 8);
      FbgGarnerParams gh{w, n, c->fb.d_m0, c->fb.d_m8, c->fb.d_coefR, c->fb.mprime0};
      HIPCHK(grp_launch_garner(gh, (int)std::max<long long>(1, std::min<long long>(gb4, (long long)occH * c->cus)), st));
      // c = w_q + q^2 h on lanes (kernels_sgp.hpp k_sgp_fin): its intermediates' top 2S rows go to the digit buffer
      // (2K rows, dead by now; K >= S at every window the ladder has)
      if (c->fb.d_sgp_q && c->ct_words == SGPF_CT_WORDS && K >= SGP_S && sgp_fin_enabled()) {
        const SgpFinParams sf{w, digits, n, c->fb.d_sgp_q, sl.dst.ct, c->ct_words};
        HIPCHK(sgp_launch_fin(sf, c->cus, st));
      } else {
        FbgFinParams gf{w, SB, n, c->d_N, c->fb.d_q2Rn, c->mprime_N, sl.dst.ct, c->ct_words};
        HIPCHK(grp_launch_fin(gf, (int)std::max<long long>(1, std::min<long long>(gb8, (long long)occC * c->cus)), st));
      }
      stage_mark(c, 3, st);
      continue;
    }
    if (c->fb.pair_s) {   // Garner on pairs (kernels_fbp.hpp)
      int occP = 1;
      fbp_fin_occupancy(c->fb.pair_s, &occP);
      FbpFinParams pp{w, n, c->fb.d_fbp_fin_p, c->fb.d_fbp_fin_cs, c->fb.fbp_fin_mprime, sl.dst.ct,
                      c->ct_words};
      pp.g = guard_args(c, 0, 0, (unsigned long long)n * c->ct_words, w_words);
      const long long nb = (n + LANE_BLOCK - 1) / LANE_BLOCK;
      HIPCHK(fbp_launch_fin(c->fb.pair_s, pp, (int)std::max<long long>(1, std::min<long long>(nb, (long long)occP * c->cus)), st));
      stage_mark(c, 3, st);
      continue;
    }
  }
  return 0;
}

// ------------------------------------------------------------------ public-key fixed bases (kernels_pfb.hpp)
// A party without the private key samples r = g_0^e_0 g_1^e_1 ... g_32^e_32 mod n from 33 bases it drew itself
// (g_0 with Jacobi symbol -1) and exponents from the element's ChaCha20 stream (e_0: nb + 64 bits, e_j: 96 bits),
// and gets r^n mod n^2 as a product of table rows (distribution argument, break-even). The rows and
// k_pe_fin's output are 64-word pairs, so of setup_pe's 1537..2048 bits only the keys of 128 ciphertext words (n of
// 2033..2048 bits) qualify, as for k_pe_* in encrypt_route.hpp.
static bool pfb_supported(const pai_ctx* c) {
  return c->pe_ok && c->ct_words == 2 * PFB_PW && (size_t)c->nb + 24 <= (size_t)LB * PFB_S;
}

static void pfb_digit_counts(const pai_ctx* c, int W, int* K0, int* KS) {
  *K0 = (c->nb + PFB_E0_EXTRA + W - 1) / W;
  *KS = (PFB_TBITS + W - 1) / W;
}

static uint64_t pfb_bytes(const pai_ctx* c, int W) {
  int K0, KS;
  pfb_digit_counts(c, W, &K0, &KS);
  return (uint64_t)(K0 + PFB_SHORT * KS) * (1ull << W) * PFB_ROW4 * 16ull;
}

static int pfb_choose_window(pai_ctx* c) {
  if (!c->pfb_W) c->pfb_W = pfb_default_window();
  const uint64_t budget = fb_budget(c);
  for (int w : {20, 16, 12})
    if (w <= c->pfb_W && pfb_bytes(c, w) <= budget) return w;
  return 0;
}

static int pfb_unavailable(pai_ctx* c, const std::string& why) {
  c->pfb.release();
  (void)hipGetLastError();
  c->pfb_state = pai_ctx::FB_UNAVAILABLE;
  c->pfb_reason = why;
  return 0;
}

// Jacobi symbol (a | n) for odd n > 0: halvings (second supplement), swaps (reciprocity), subtractions
static int jacobi(HBig a, HBig n) {
  if (cmp(a, n) >= 0) a = mod(a, n);
  int t = 1;
  while (!a.is_zero()) {
    while (!a.is_odd()) {
      a = shr1(a);
      const uint32_t r = n.w[0] & 7u;
      if (r == 3 || r == 5) t = -t;
    }
    if (cmp(a, n) < 0) {
      std::swap(a, n);
      if ((a.w[0] & 3u) == 3u && (n.w[0] & 3u) == 3u) t = -t;
    }
    a = sub(a, n);
  }
  return (n.w.size() == 1 && n.w[0] == 1u) ? t : 0;
}

// uniform in [2, n) from the OS CSPRNG (rejection sampling on bits(n) bits)
static bool random_below(const HBig& n, HBig* out) {
  const size_t nw = n.w.size();
  const int top = (int)(n.bits() - 32 * (nw - 1));
  for (int tries = 0; tries < 1000; ++tries) {
    HBig r;
    r.w.assign(nw, 0);
    size_t got = 0;
    while (got < nw * 4) {
      const ssize_t k = getrandom((char*)r.w.data() + got, nw * 4 - got, 0);
      if (k <= 0) return false;
      got += (size_t)k;
    }
    if (top < 32) r.w[nw - 1] &= (1u << top) - 1u;
    r.trim();
    if (cmp(r, n) < 0 && r.bits() > 1) {
      *out = r;
      return true;
    }
  }
  return false;
}

// g_0 with Jacobi symbol -1 (so that the publicly visible symbol of c mod n is uniform) and PFB_SHORT further bases,
// unless the caller set them (pai_ctx_public_fb_set_bases)
static bool pfb_draw_bases(pai_ctx* c) {
  if (!c->pfb_bases.empty()) return true;
  std::vector<HBig> bs;
  HBig g;
  do {
    if (!random_below(c->n, &g)) return false;
  } while (jacobi(g, c->n) != -1);
  bs.push_back(g);
  for (int j = 0; j < PFB_SHORT; ++j) {
    if (!random_below(c->n, &g)) return false;
    bs.push_back(g);
  }
  c->pfb_bases = bs;
  return true;
}

// The public tables' constants, scratch and table on the device (the modulus is n: one "half" of the pair-group builder)
static int pfb_upload(pai_ctx* c, int W, int K0, int KS, RowScratch& sc, uint4** table) {
  SetupTrace tr_m("  pfb uploads + hipMalloc");
  const HBig &n = c->n, &n2 = c->N;
  const size_t RS = (size_t)LB * PFB_S;
  const int K = K0 + PFB_SHORT * KS;
  PfbTables& pfb = c->pfb;
  const HBig oneR = mul_pow2_mod(HBig(1), RS, n2);
  const HBig X = mod(sub(add(n, HBig(1)), mul_pow2_mod(HBig(1), RS, n)), n);   // (1 - R) mod n
  std::vector<uint32_t> gl;
  for (const HBig& g : c->pfb_bases) append(gl, g.limbs(PFB_S, LB));
  uint32_t *dn, *dx, *done, *dr2, *dgl, *dnw;
  int rc;
  if ((rc = upload_to(pfb.mem, n.limbs(PFB_S, LB), &dn)) || (rc = upload_to(pfb.mem, X.limbs(PFB_S, LB), &dx)) ||
      (rc = upload_to(pfb.mem, pair_split(oneR, n, PFB_S), &done)) ||
      (rc = upload_to(pfb.mem, pair_split(mul_pow2_mod(oneR, RS, n2), n, PFB_S), &dr2)) ||
      (rc = upload_to(pfb.mem, gl, &dgl)) || (rc = upload_to(pfb.mem, n.words(PFB_PW), &dnw)))
    return rc;
  if (!sc.alloc(K, W, PFB_S, true) ||
      !(*table = (uint4*)TableArena::get().alloc(c->device, ((size_t)K << W) * PFB_ROW4 * sizeof(uint4))))
    return fail(PAI_ERR_HIP, "table allocation failed");
  pfb.tables.push_back(*table);
  PfbConst pc{};
  pc.g = FbgpHalf{(const uint32_t*)*table, dn, dx, done, sc.bases, sc.lohi, nullptr, nullptr, nullptr, nullptr,
                  mont_prime(n, LB), 0u, sc.inv, sc.pre, sc.cval};
  pc.table = *table;
  pc.gl = dgl;
  pc.r2 = dr2;
  pc.nw = dnw;
  pc.nbits = (int)n.bits();
  pc.nbases = (int)c->pfb_bases.size();
  pc.K = K;
  pc.W = W;
  pc.K0 = K0;
  pc.KS = KS;
  if ((rc = upload_to(pfb.mem, std::vector<PfbConst>{pc}, &pfb.d_pfb))) return rc;
  if (sgp_enabled()) {
    SgpHalf sh{};
    if ((rc = sgp_make_half(n, HBig(1), K, *table, pfb.mem, &sh)) ||
        (rc = upload_to(pfb.mem, std::vector<SgpHalf>{sh}, &pfb.d_sgp)))
      return rc;
  }
  return 0;
}

static int ensure_pfb(pai_ctx* c) {
  if (c->pfb_state == pai_ctx::FB_READY) return 1;
  if (c->pfb_state == pai_ctx::FB_UNAVAILABLE) return 0;
  if (!pfb_supported(c)) return pfb_unavailable(c, "the public fixed-base kernels need an n of 2033..2048 bits (128 ciphertext words)");
  const int W = pfb_choose_window(c);
  if (!W) return pfb_unavailable(c, "tables do not fit the device memory budget");
  SetupTrace tr_all("ensure_pfb");
  int K0, KS;
  pfb_digit_counts(c, W, &K0, &KS);
  const int K = K0 + PFB_SHORT * KS;
  {
    SetupTrace tr_h("  pfb host prep (bases, constants)");
    if (!pfb_draw_bases(c)) return pfb_unavailable(c, "no randomness for the bases");
  }
  PfbTables& pfb = c->pfb;
  pfb.release();
  RowScratch sc;
  uint4* table = nullptr;
  if (pfb_upload(c, W, K0, KS, sc, &table)) return pfb_unavailable(c, pai_last_error());
  static const char* const lab[3] = {"  pfb phase 1 (chains, lohi, inv_fwd)", "  pfb host invert", "  pfb phase 2 (inv_bwd, fill)"};
  if (build_factored_rows(
          lab, [&] { return pfb_build_phase1(pfb.d_pfb, (int)c->pfb_bases.size(), K, W, nullptr); },
          [&] { return pfb_build_phase2(pfb.d_pfb, K, W, table, nullptr); }, &c->n, &sc, 1, K, PFB_S))
    return pfb_unavailable(c, pai_last_error());
  {
    SetupTrace tr_f("  pfb scratch frees");
    sc.free();
  }
  pfb.K = K;
  pfb.K0 = K0;
  pfb.W_used = W;
  c->pfb_state = pai_ctx::FB_READY;
  return 1;
}

// Break-even of the public tables, from measurements on one MI355X (tools/pfb_breakeven.py): the build takes 0.114 s +
// 1.91 ns per row on memory the process has not released before (0.117 / 0.155 / 0.648 s at W = 12 / 16 / 20, round 5,
// profiles/r05_pfb_breakeven_before.json; round 6: 0.094 / 0.137 s at W = 12 / 16), and each element then costs
// 1 / rate(W) on k_sgp (round 6, the final library: 3.00 M / 3.93 M / 4.78 M enc/s, profiles/r06e_pfb_breakeven.json)
// instead of 1 / 552 k on the factored k_pe_* chain (round 5's 503 k predated that chain) -- 1.81 us -- so the
// break-even is ~100 k elements at the default W = 16
static long long pfb_threshold(pai_ctx* c) {
  if (c->pfb_state != pai_ctx::FB_UNTRIED || !pfb_supported(c)) return 0;
  if (const char* e = getenv("FLEXPAI_PFB_MIN_ELEMS")) return atoll(e);
  const int W = pfb_choose_window(c);
  if (!W) return 0;
  int K0, KS;
  pfb_digit_counts(c, W, &K0, &KS);
  const double build_s = 0.114 + (double)(K0 + PFB_SHORT * KS) * (double)(1ull << W) * 1.91e-9;
  const double rate = W >= 20 ? 4.78e6 : W >= 16 ? 3.93e6 : 3.00e6;
  const double save_s = 1.0 / 5.52e5 - 1.0 / rate;
  return (long long)(build_s / save_s) + 1;
}

static bool pfb_wanted(pai_ctx* c, long long n) {
  if (c->pfb_state != pai_ctx::FB_UNTRIED) return true;
  if (c->pfb_call) return c->pfb_call > 0;
  c->pfb_seen += n;
  return c->pfb_seen >= pfb_threshold(c);
}

// digits, k_pfb, k_pe_fin per chunk of CRT_CHUNK elements
static int launch_pfb(pai_ctx* c, const EncParams& e, hipStream_t st) {
  const long long N = e.n;
  const long long chunk = std::min(N, CRT_CHUNK);
#if FLEXPAI_XCHECK
  int occ = 1;
  pfb_occupancy(&occ);
  constexpr int GPB = BLOCK / PFB_TPI;
  const int gx = (int)std::max<long long>(1, std::min<long long>((chunk + GPB - 1) / GPB, (long long)occ * c->cus));
#else
  if (!c->pfb.d_sgp) return fail(PAI_ERR_KEY, "public fixed-base encrypt: no split-pair tables");
#endif
  const size_t dbytes = (size_t)c->pfb.K * 4, xbytes = (size_t)2 * PFB_SP * 4;
  int rc;
  if ((rc = ensure_work(c, (dbytes + xbytes) * chunk))) return rc;
  uint32_t* digits = (uint32_t*)c->d_work;
  uint32_t* xw = (uint32_t*)((char*)c->d_work + dbytes * chunk);
  for (long long off = 0; off < N; off += chunk) {
    const long long n = std::min(chunk, N - off);
    const EncSlice sl = enc_slice(e, off);
    PfbDigitParams pd{};
    pd.n = n;
    std::memcpy(pd.rng_key, sl.rnd.rng_key, sizeof(pd.rng_key));
    pd.index_base = sl.rnd.index_base;
    pd.K = c->pfb.K;
    pd.W = c->pfb.W_used;
    pd.digits = digits;
    const int gD = (int)std::max<long long>(1, std::min<long long>((long long)8 * c->cus, (n + PFB_DIG_BLOCK - 1) / PFB_DIG_BLOCK));
    stage_mark(c, 0, st);
    HIPCHK(pfb_launch_digits(pd, gD, st));
    stage_mark(c, 1, st);
    const PfbParams pp{c->pfb.d_pfb, n, digits, sl.src, sl.dst, xw};
    if (c->pfb.d_sgp) {   // split pairs (kernels_sgp.hpp)
      int occS = 1;
      sgp_occupancy(&occS);
      SgpParams sp{c->pfb.d_sgp, n, c->pfb.K, c->pfb.W_used, digits, xw, sl.src, sl.dst};
      sp.g = guard_args(c, (unsigned long long)c->pfb.K << c->pfb.W_used, (unsigned long long)c->pfb.K * chunk,
                        (unsigned long long)2 * PFB_SP * chunk, 0);
      const long long nb = (n + SGP_PAIRS - 1) / SGP_PAIRS;
      HIPCHK(sgp_launch(sp, (int)std::max<long long>(1, std::min<long long>(nb, (long long)occS * c->cus)), 1, st));
    } else {
#if FLEXPAI_XCHECK
      HIPCHK(pfb_launch(pp, (int)std::min<long long>(gx, (n + GPB - 1) / GPB), st));
#endif
    }
    stage_mark(c, 2, st);
    PeParams pf{};
    pf.k = c->d_pe;
    pf.n = n;
    pf.xw = xw;
    pf.ct = sl.dst.ct;
    pf.ct_words = sl.dst.ct_words;
    HIPCHK(pe_launch_fin(pf, c->cus, st));
    stage_mark(c, 3, st);
  }
  return 0;
}

int pai_ctx_public_fb_prepare(pai_ctx* c) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  HIPCHK(hipSetDevice(c->device));
  if (!ensure_pfb(c)) return fail(PAI_ERR_KEY, "public fixed-base obfuscation not available: " + c->pfb_reason);
  return 0;
}

int pai_ctx_public_fb_set_bases(pai_ctx* c, const uint8_t* bases_le, size_t base_bytes, int nbases) {
  if (!c || !bases_le || base_bytes == 0) return fail(PAI_ERR_ARG, "pai_ctx_public_fb_set_bases: null argument");
  CtxLock lk(c);
  if (nbases != PFB_NBASES) return fail(PAI_ERR_ARG, "pai_ctx_public_fb_set_bases: wrong number of bases");
  std::vector<HBig> bs;
  for (int j = 0; j < nbases; ++j) {
    HBig g = HBig::from_le_bytes(bases_le + (size_t)j * base_bytes, base_bytes);
    if (g.bits() < 2 || cmp(g, c->n) >= 0) return fail(PAI_ERR_ARG, "pai_ctx_public_fb_set_bases: need 1 < g < n");
    // the distribution argument needs units, g_0 with Jacobi symbol -1 (so that (c mod n | n) is
    // uniform) and distinct bases: reject anything weaker rather than sample a visibly biased r
    if (inv_mod(g, c->n).is_zero()) return fail(PAI_ERR_ARG, "pai_ctx_public_fb_set_bases: a base is not a unit mod n");
    for (const HBig& h : bs)
      if (cmp(h, g) == 0) return fail(PAI_ERR_ARG, "pai_ctx_public_fb_set_bases: repeated base");
    if (j == 0 && jacobi(g, c->n) != -1)
      return fail(PAI_ERR_ARG, "pai_ctx_public_fb_set_bases: g_0 must have Jacobi symbol -1 mod n");
    bs.push_back(g);
  }
  HIPCHK(hipSetDevice(c->device));
  c->pfb.release();
  c->pfb_bases = bs;
  c->pfb_state = pai_ctx::FB_UNTRIED;
  return 0;
}

int pai_ctx_public_fb_info(pai_ctx* c, uint8_t* bases_le, size_t base_bytes, int* nbases, int* digits, int* window,
                           int* e0_digits) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (c->pfb_state != pai_ctx::FB_READY) return fail(PAI_ERR_KEY, "public fixed-base tables are not resident");
  if (bases_le) {
    for (size_t j = 0; j < c->pfb_bases.size(); ++j) {
      const std::vector<uint32_t> w = c->pfb_bases[j].words((base_bytes + 3) / 4);
      if (c->pfb_bases[j].bits() > 8 * base_bytes) return fail(PAI_ERR_ARG, "pai_ctx_public_fb_info: base_bytes too small");
      std::memcpy(bases_le + j * base_bytes, w.data(), base_bytes);
    }
  }
  if (nbases) *nbases = (int)c->pfb_bases.size();
  if (digits) *digits = c->pfb.K;
  if (window) *window = c->pfb.W_used;
  if (e0_digits) *e0_digits = c->pfb.K0;
  return 0;
}

int pai_ctx_public_fb_policy(pai_ctx* c, long long* seen, long long* threshold) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (seen) *seen = c->pfb_seen;
  if (threshold) *threshold = pfb_threshold(c);
  return 0;
}

// public-key encryption on split pairs (kernels_pe.hpp, engine_pe.hip), in chunks of CRT_CHUNK elements
// the modulus of a batch inversion on the group engine: n^2 (ciphertexts, TPI = tpi_e) or n (the public-key chain's
// bases, TPI = 2)
struct InvMod {
  int tpi, W, S;             // group size, words per value, limbs (TPI L)
  const uint32_t *N, *R2, *oneR;
  uint32_t mprime;
  const HBig* mod;
};
static int batch_invert(pai_ctx* c, uint32_t* x, const uint8_t* flag, long long n, hipStream_t st, const InvMod& md);
static int batch_invert(pai_ctx* c, uint32_t* x, const uint8_t* flag, long long n, hipStream_t st);
static int batch_invert_async(pai_ctx* c, uint32_t* x, long long n, hipStream_t st, const InvMod& md, uint32_t** d_noinv);

// Chunks below this many elements take the general chain: the factored one saves ~0.2 us per element (k_pe_pow_f
// against k_pe_pow) and costs the batch inversion's fixed ~1-2 ms of short dependent launches. $FLEXPAI_PEF_MIN
// overrides (the parity tests force both chains on the same inputs).
static long long pef_min_elems() {
  if (const char* e = getenv("FLEXPAI_PEF_MIN")) return atoll(e);
  return 16384;
}

// public-key encryption for n <= 1024 bits on pairs (kernels_pe1.hpp, engine_pe1.hip), in chunks of CRT_CHUNK elements;
// stage times: the obfuscator words + k_dec_pre_pair, k_pe1_pow, k_pe1_fin
static int launch_pe1(pai_ctx* c, const EncParams& e, hipStream_t st) {
  const long long N = e.n;
  const long long chunk = std::min(N, CRT_CHUNK);
  const int RW = enc_r_words(e);
  const int kchunks = 2;   // r's digits in two chunks of S (zeros past its words): the constant is the pair of R^3
  if (RW <= 0 || 32 * RW > kchunks * LB * PE1_S) return fail(PAI_ERR_ARG, "1024-bit pair encrypt: obfuscator too wide");
  int occ = 1;
  pe1_occupancy(&occ);
  const long long lb = (chunk + LANE_BLOCK - 1) / LANE_BLOCK;
  const int gx = (int)std::max<long long>(1, std::min<long long>(lb, (long long)occ * c->cus));
  int rc = ensure_scratch(c, (size_t)gx * LANE_BLOCK * lane_scratch_words<2 * PE1_S>() * 4);
  if (rc) return rc;
  const size_t rwb = (size_t)RW * 4, xwb = (size_t)2 * PE1_S * 4;   // per element
  if ((rc = ensure_work(c, (rwb + xwb) * chunk))) return rc;
  for (long long off = 0; off < N; off += chunk) {
    const long long n = std::min(chunk, N - off);
    hipEvent_t* ev = stage_chunk(c);
    if (ev) c->nev = 4;
    Pe1Params p{};
    set_flat(p, enc_slice(e, off));
    p.n = n;
    p.nl = c->d_pe1_n;
    p.one = c->d_pe1_one;
    p.prog = c->d_pe1_prog;
    p.nprog = c->pe1_nprog;
    p.r2n = c->d_pe1_r2n;
    p.mprime = c->pe1_mprime;
    p.rw = (uint32_t*)c->d_work;
    p.rw_words = RW;
    p.xw = (uint32_t*)((char*)c->d_work + rwb * chunk);
    p.scratch = (uint32_t*)c->d_scratch;
    const DecPairPreParams pre{c->d_pe1_half, n, p.rw, RW, kchunks, p.xw};
    HIPCHK(pe1_launch(p, pre, gx, c->cus, st, ev));
  }
  return 0;
}

static int launch_pe(pai_ctx* c, const EncParams& e, hipStream_t st) {
  const long long N = e.n;
  const long long chunk = std::min(N, CRT_CHUNK);
  Dec4Geom g;
  pe_geometry(c->cus, chunk, &g);
  int rc = ensure_scratch(c, g.scratch_bytes);
  if (rc) return rc;
  const size_t xbytes = (size_t)2 * D4_S * 4;   // per element, + 8 for M
  const size_t awbytes = c->pef_ok ? (size_t)c->pt_words * 4 : 0, iobytes = c->pef_ok ? (size_t)D4_S * 4 : 0;
  if ((rc = ensure_work(c, (xbytes + 8 + awbytes + iobytes) * chunk))) return rc;
  for (long long off = 0; off < N; off += chunk) {
    const long long n = std::min(chunk, N - off);
    hipEvent_t* ev = stage_chunk(c);
    if (ev) c->nev = 4;
    PeParams p{};
    p.k = c->d_pe;
    set_flat(p, enc_slice(e, off));
    p.n = n;
    p.xw = (uint32_t*)c->d_work;
    p.M = (int64_t*)((char*)c->d_work + xbytes * chunk);
    p.scratch = (uint32_t*)c->d_scratch;
    if (!c->pef_ok || n < pef_min_elems()) {
      HIPCHK(pe_launch(p, g, st, ev));
      continue;
    }
    // the factored chain: A_r's batch inversion mod n (one host inversion per chunk), iota, k_pe_pow_f
    p.aw = (uint32_t*)((char*)c->d_work + (xbytes + 8) * chunk);
    p.aw_words = c->pt_words;
    p.iota = (uint32_t*)((char*)p.aw + awbytes * chunk);
    HIPCHK(pe_launch_pre_aw(p, g, st, ev));
    uint32_t* noinv = nullptr;
    rc = batch_invert_async(c, p.aw, n, st,
                            InvMod{2, c->pt_words, 2 * L, c->d_pe_n, c->d_pe_r2, c->d_pe_oneR, c->pe_mprime, &c->n}, &noinv);
    if (rc) return rc;
    // an A_r that shares a factor with n (no inverse): the device flag sends this chunk down the general chain
    p.noinv = noinv;
    HIPCHK(pe_launch_iota_pow_f(p, g, st, ev));
  }
  return 0;
}

// public-key encryption for n of 2049..4096 bits on pair groups (kernels_pe4.hpp, engine_pe4.hip), in chunks of CRT_CHUNK
// elements; stage times: k_pe4_pre, k_pe4_pow, k_pe4_fin
static int launch_pe4(pai_ctx* c, const EncParams& e, hipStream_t st) {
  const long long N = e.n;
  const long long chunk = std::min(N, CRT_CHUNK);
  const int RW = enc_r_words(e);
  if (RW <= 0 || 32 * RW > 2 * LB * PE4_S)   // r's 2 S digits (its words are staged in the same 2 S slot words)
    return fail(PAI_ERR_ARG, "4096-bit pair encrypt: obfuscator too wide");
  Pe4Geom g;
  pe4_geometry(c->cus, chunk, &g);
  int rc = ensure_scratch(c, g.scratch_bytes);
  if (rc) return rc;
  const size_t xbytes = (size_t)2 * PE4_S * 4;   // per element, + 8 for M
  if ((rc = ensure_work(c, (xbytes + 8) * chunk))) return rc;
  for (long long off = 0; off < N; off += chunk) {
    const long long n = std::min(chunk, N - off);
    hipEvent_t* ev = stage_chunk(c);
    if (ev) c->nev = 4;
    Pe4Params p{};
    p.k = c->d_pe4;
    const EncSlice sl = enc_slice(e, off);
    p.src = sl.src;
    p.rnd = sl.rnd;
    p.dst = sl.dst;
    p.n = n;
    p.xw = (uint32_t*)c->d_work;
    p.M = (int64_t*)((char*)c->d_work + xbytes * chunk);
    p.scratch = (uint32_t*)c->d_scratch;
    HIPCHK(pe4_launch(p, g, st, ev));
  }
  return 0;
}

// k_crt_fin over elements [off, off + n) of the call: c = (u_p q^2 + u_q p^2) c0 mod n^2 from u [2][sb][n]
static int crt_finish(pai_ctx* c, const EncParams& e, const uint32_t* u, int sb, long long off, long long n,
                      hipStream_t st) {
  const EncSlice sl = enc_slice(e, off);
  CrtFinParams f{};
  f.src = sl.src;
  f.dst = sl.dst;
  f.u = u;
  f.sb = sb;
  f.n = n;
  f.N = c->d_N;
  f.nl = c->d_nl;
  f.kq = c->d_kq;
  f.kp = c->d_kp;
  f.mprime = c->mprime_N;
  switch (c->tpi_e) {
    case 2: return launch_crt_fin<2>(c, f, st);
    case 4: return launch_crt_fin<4>(c, f, st);
    case 8: return launch_crt_fin<8>(c, f, st);
  }
  return fail(PAI_ERR_KEY, "CRT finish: unsupported group size");
}

// A call of at most crtw_max elements: both exponentiations on 16-lane rows (k_crt_w, kernels_crtw.hpp), then
// k_crt_fin. Same constants, op lists and output as k_crt_a + k_crt_b_pair; stage times: k_crt_w, k_crt_fin.
static int launch_crtw(pai_ctx* c, const EncParams& e, int sa, int sb, int kchunks, hipStream_t st) {
  const long long N = e.n;
  int rc = ensure_work(c, (size_t)2 * sb * 4 * N);
  if (rc) return rc;
  uint32_t* u = (uint32_t*)c->d_work;
  crtw::Params p{};
  p.ha = c->d_crt_a;
  p.hb = c->d_crt_b;
  p.n = N;
  p.rnd = enc_slice(e, 0).rnd;
  p.kchunks = kchunks;
  p.out = u;
  stage_mark(c, 0, st);
  HIPCHK(crtw_launch(sa, p, st));
  stage_mark(c, 1, st);
  if ((rc = crt_finish(c, e, u, sb, 0, N, st))) return rc;
  stage_mark(c, 2, st);
  return 0;
}

template <int SA, int SB>
static int launch_crt(pai_ctx* c, const EncParams& e, bool rows, hipStream_t st) {
  static_assert(SB == 2 * SA || SB == 2 * SA - 1, "stage sizes");
  const long long N = e.n;
  const int r_words = enc_r_words(e);
  const int kchunks = (32 * r_words + LB * SA - 1) / (LB * SA);
  if (kchunks > KMAX_CHUNKS || (e.obf == PAI_OBF_RNG && r_words > RBUF_WORDS))
    return fail(PAI_ERR_ARG, "CRT encrypt: obfuscator too wide");
  if (rows) return launch_crtw(c, e, SA, SB, kchunks, st);
  const long long chunk = std::min(N, CRT_CHUNK);
  int occA = 1, occB = 1;
  if (crt_lane_occupancy(SA, &occA, &occB)) return fail(PAI_ERR_KEY, "CRT encrypt: unsupported size");
  const bool bpair = c->crt_pair_ok;   // stage B on pairs (kernels_pair.hpp)
#if !FLEXPAI_XCHECK
  if (!bpair) return fail(PAI_ERR_KEY, "CRT encrypt: no pair constants");
#endif
  if (bpair && crt_b_pair_occupancy(SA, &occB)) return fail(PAI_ERR_KEY, "CRT encrypt: unsupported size");
  const long long lanes_blocks = (chunk + LANE_BLOCK - 1) / LANE_BLOCK;
  const int gxA = (int)std::max<long long>(1, std::min<long long>(lanes_blocks, (long long)occA * c->cus / 2));
  const int gxB = (int)std::max<long long>(1, std::min<long long>(lanes_blocks, (long long)occB * c->cus / 2));
  const size_t scrA = (size_t)2 * gxA * LANE_BLOCK * lane_scratch_words<SA>() * 4;
  const size_t scrB = (size_t)2 * gxB * LANE_BLOCK * lane_scratch_words<SB>() * 4;
  int rc = ensure_scratch(c, std::max(scrA, scrB));
  if (rc) return rc;
  const size_t ybytes = (size_t)2 * SA * 4;   // per element
  if ((rc = ensure_work(c, (ybytes + (size_t)2 * SB * 4) * chunk))) return rc;
  uint32_t* y = (uint32_t*)c->d_work;
  uint32_t* u = (uint32_t*)((char*)c->d_work + ybytes * chunk);
  for (long long off = 0; off < N; off += chunk) {
    const long long n = std::min(chunk, N - off);
    CrtParams pa{};
    pa.halves = c->d_crt_a;
    pa.n = n;
    pa.rnd = enc_slice(e, off).rnd;
    pa.kchunks = kchunks;
    pa.out = y;
    pa.scratch = (uint32_t*)c->d_scratch;
    const int gA = (int)std::min<long long>(gxA, (n + LANE_BLOCK - 1) / LANE_BLOCK);
    stage_mark(c, 0, st);
    HIPCHK(crt_launch_a(SA, pa, gA, st));
    stage_mark(c, 1, st);
    HIPCHK(hipGetLastError());
    CrtParams pb{};
    pb.halves = bpair ? c->d_crtp_b : c->d_crt_b;
    pb.n = n;
    pb.yin = y;
    pb.out = u;
    pb.scratch = (uint32_t*)c->d_scratch;
    const int gB = (int)std::min<long long>(gxB, (n + LANE_BLOCK - 1) / LANE_BLOCK);
    HIPCHK(crt_b_pair_launch(SA, pb, gB, st));
    HIPCHK(hipGetLastError());
    stage_mark(c, 2, st);
    if ((rc = crt_finish(c, e, u, SB, off, n, st))) return rc;
    stage_mark(c, 3, st);
  }
  return 0;
}

// A 2049..4096-bit key holder's call above the rows: k_crt4_pre + k_crt4_a (stage A, one element-half per lane),
// k_crt4_b (stage B on split pairs), k_crt_fin<8>, in chunks of CRT4_CHUNK elements (y and u: 1776 B per element,
// 466 MB per chunk; CRT_CHUNK's 4 M would make it 7.4 GB). Stage times: stage A, stage B, finish, summed over chunks.
constexpr long long CRT4_CHUNK = 1ll << 18;
static int launch_crt4(pai_ctx* c, const EncParams& e, hipStream_t st) {
  constexpr int S = D4_S;
  const long long N = e.n;
  const int r_words = enc_r_words(e);
  const int kchunks = (32 * r_words + LB * S - 1) / (LB * S);
  if (kchunks > KMAX_CHUNKS || (e.obf == PAI_OBF_RNG && r_words > RBUF_WORDS))
    return fail(PAI_ERR_ARG, "CRT encrypt: obfuscator too wide");
  const long long chunk = std::min(N, CRT4_CHUNK);
  Crt4Geom g;
  crt4_geometry(c->cus, chunk, &g);
  int rc = ensure_scratch(c, g.scratch_bytes);
  if (rc) return rc;
  const size_t ybytes = (size_t)2 * S * 4;   // per element
  if ((rc = ensure_work(c, (ybytes + (size_t)2 * 2 * S * 4) * chunk))) return rc;
  uint32_t* y = (uint32_t*)c->d_work;
  uint32_t* u = (uint32_t*)((char*)c->d_work + ybytes * chunk);
  for (long long off = 0; off < N; off += chunk) {
    const long long n = std::min(chunk, N - off);
    Crt4Params p{};
    p.ha = c->d_crt_a;
    p.hb = c->d_crt4_b;
    p.n = n;
    p.rnd = enc_slice(e, off).rnd;
    p.kchunks = kchunks;
    p.y = y;
    p.u = u;
    p.scratch = (uint32_t*)c->d_scratch;
    stage_mark(c, 0, st);
    HIPCHK(crt4_launch_a(p, g, st));
    HIPCHK(hipGetLastError());
    stage_mark(c, 1, st);
    HIPCHK(crt4_launch_b(p, g, st));
    HIPCHK(hipGetLastError());
    stage_mark(c, 2, st);
    if ((rc = crt_finish(c, e, u, 2 * S, off, n, st))) return rc;
    stage_mark(c, 3, st);
  }
  return 0;
}

static int encrypt_dev(pai_ctx* c, int dtype, const void* d_x, size_t N, int exp_mode, int32_t fixed_exp, int obf_mode,
                       const uint32_t* d_r_words, size_t r_stride_words, size_t r_words, const uint8_t* rng_key32,
                       uint64_t index_base, uint32_t* d_ct, int32_t* d_exp, int32_t* d_status, hipStream_t st);
static int pool_encrypt_dev(pai_ctx* c, int dtype, const void* d_x, size_t N, int exp_mode, int32_t fixed_exp,
                            uint32_t* d_ct, int32_t* d_exp, int32_t* d_status, hipStream_t st);
static int pool_check_take(pai_ctx* c, size_t N, const char* who);

int pai_encrypt_dev(pai_ctx* c, int dtype, const void* d_x, size_t N, int exp_mode, int32_t fixed_exp, int obf_mode,
                    const uint32_t* d_r_words, size_t r_stride_words, size_t r_words, const uint8_t* rng_key32,
                    uint64_t index_base, uint32_t* d_ct, int32_t* d_exp, int32_t* d_status, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  if (N == 0) return 0;
  if (dtype < 0 || dtype > 2 || !d_x || !d_ct || !d_exp) return fail(PAI_ERR_ARG, "pai_encrypt_dev: bad arguments");
  if (obf_mode == PAI_OBF_GIVEN && (!d_r_words || r_words == 0 || r_words > (size_t)c->ct_words))
    return fail(PAI_ERR_ARG, "pai_encrypt_dev: r must be given with 0 < r_words <= ct_words");
  if (obf_mode == PAI_OBF_RNG && !rng_key32) return fail(PAI_ERR_ARG, "pai_encrypt_dev: rng key required");
  if (obf_mode == PAI_OBF_POOL)
    return pool_encrypt_dev(c, dtype, d_x, N, exp_mode, fixed_exp, d_ct, d_exp, d_status, (hipStream_t)stream);
  if (obf_mode < 0 || obf_mode > 2) return fail(PAI_ERR_ARG, "pai_encrypt_dev: bad obf_mode");
  return encrypt_dev(c, dtype, d_x, N, exp_mode, fixed_exp, obf_mode, d_r_words, r_stride_words, r_words, rng_key32,
                     index_base, d_ct, d_exp, d_status, (hipStream_t)stream);
}

// pai_encrypt_dev below its argument checks (the caller holds the context's lock): the route, the samplers' break-even
// counters and tables, the launches. pai_obfuscate_dev runs it on zeros for its r^n.
static int encrypt_dev(pai_ctx* c, int dtype, const void* d_x, size_t N, int exp_mode, int32_t fixed_exp, int obf_mode,
                       const uint32_t* d_r_words, size_t r_stride_words, size_t r_words, const uint8_t* rng_key32,
                       uint64_t index_base, uint32_t* d_ct, int32_t* d_exp, int32_t* d_status, hipStream_t st) {
  HIPCHK(hipSetDevice(c->device));
  stage_reset(c);
  EncParams p{};
  p.x = d_x;
  p.dtype = dtype;
  p.exp_mode = exp_mode;
  p.fexp = fixed_exp;
  p.obf = obf_mode;
  p.r = d_r_words;
  p.r_stride = (long long)r_stride_words;
  p.r_words = (int)r_words;
  p.rng_words = rng_stream_words(c);
  if (rng_key32)
    for (int i = 0; i < 8; ++i) std::memcpy(&p.rng_key[i], rng_key32 + 4 * i, 4);
  p.index_base = index_base;
  p.ct = d_ct;
  p.exp = d_exp;
  p.status = d_status;
  p.n = (long long)N;
  p.N = c->d_N;
  p.R2 = c->d_R2;
  p.nl = c->d_nl;
  p.mprime = c->mprime_N;
  p.prog = c->d_prog;
  p.nprog = c->nprog;
  p.ct_words = c->ct_words;
  const int r_eff = enc_r_words(p);
  const EncryptRoute rt = encrypt_route(route_facts(c), obf_mode, p.n, r_eff);
  // the impure steps: a call counts towards a sampler's break-even, and builds its tables, only for the sampler named
  if (rt.sampler == PAI_SAMPLER_KEY && fb_wanted(c, p.n) && ensure_fb(c)) {
    const int rc = launch_fb(c, p, st);
    return rc ? rc : guard_collect(c, st);
  }
  if (rt.sampler == PAI_SAMPLER_PUBLIC && pfb_wanted(c, p.n) && ensure_pfb(c)) {
    const int rc = launch_pfb(c, p, st);
    return rc ? rc : guard_collect(c, st);
  }
  switch (rt.chain) {
    case PAI_CHAIN_CRT_ROWS4:
      return launch_crtw(c, p, c->rows_sa, 2 * c->rows_sa, (32 * r_eff + LB * c->rows_sa - 1) / (LB * c->rows_sa), st);
    case PAI_CHAIN_CRT_ROWS:
    case PAI_CHAIN_CRT_LANE:
      return c->crt_sa == 19 ? launch_crt<19, 37>(c, p, rt.chain == PAI_CHAIN_CRT_ROWS, st)
                             : launch_crt<37, 74>(c, p, rt.chain == PAI_CHAIN_CRT_ROWS, st);
    case PAI_CHAIN_CRT4: return launch_crt4(c, p, st);
    case PAI_CHAIN_PE_ROWS:
      stage_mark(c, 0, st);
      HIPCHK(pew_launch(c->S_e, p, c->d_pew_prog, c->pew_nprog, st));
      stage_mark(c, 1, st);
      return 0;
    case PAI_CHAIN_PE: return launch_pe(c, p, st);
    case PAI_CHAIN_PE1: return launch_pe1(c, p, st);
    case PAI_CHAIN_PE4: return launch_pe4(c, p, st);
  }
  switch (c->tpi_e) {
    case 2: return launch_encrypt<2>(c, p, st);
    case 4: return launch_encrypt<4>(c, p, st);
    case 8: return launch_encrypt<8>(c, p, st);
  }
  return fail(PAI_ERR_KEY, "unsupported group size");
}

// ------------------------------------------------------------------ re-randomisation (kernels_obf.hpp)
// One sampler decision and one stage-timing record for every slice or chunk of a pai_obfuscate[_dev] call, as HostCall
// keeps them for pai_encrypt's chunks: the bits of a call do not depend on how it is cut. Nested (the host-buffer
// call around its chunks' device calls) the outer scope's decision stands and only the outer scope drops it.
struct ObfCall {
  pai_ctx* c;
  bool own_keep = false, own_fb = false, own_pfb = false;
  ObfCall(pai_ctx* ctx, int obf_mode, long long N) : c(ctx) {
    if (!c->stage_keep) {
      stage_reset(c);
      c->stage_keep = own_keep = true;
    }
    if (obf_mode != PAI_OBF_RNG || c->fb_call || c->pfb_call) return;
    const int sampler = encrypt_route(route_facts(c), obf_mode, N, rng_stream_words(c)).sampler;
    if (sampler == PAI_SAMPLER_KEY) {
      c->fb_call = fb_wanted(c, N) ? 1 : -1;
      own_fb = true;
    } else if (sampler == PAI_SAMPLER_PUBLIC) {
      c->pfb_call = pfb_wanted(c, N) ? 1 : -1;
      own_pfb = true;
    }
  }
  ~ObfCall() {
    if (own_keep) c->stage_keep = false;
    if (own_fb) c->fb_call = 0;
    if (own_pfb) c->pfb_call = 0;
  }
};

// out <- ct s mod n^2 over n elements (out may be ct or s)
static int launch_obf_mul(pai_ctx* c, const uint32_t* ct, const uint32_t* s, uint32_t* out, long long n, hipStream_t st) {
  int occ = 1;
  if (obf_occupancy(c->tpi_e, &occ)) return fail(PAI_ERR_KEY, "unsupported group size");
  const int gpb = BLOCK / c->tpi_e;
  const int grid = (int)std::max<long long>(1, std::min<long long>((n + gpb - 1) / gpb, (long long)occ * c->cus));
  ObfMulParams p{};
  p.c = ct;
  p.s = s;
  p.out = out;
  p.n = n;
  p.N = c->d_N;
  p.R2 = c->d_R2;
  p.mprime = c->mprime_N;
  p.ct_words = c->ct_words;
  HIPCHK(obf_launch(c->tpi_e, p, grid, st));
  return 0;
}

static int pool_obfuscate_dev(pai_ctx* c, const uint32_t* d_ct, size_t N, uint32_t* d_out, hipStream_t st);

// r^n is the encryption of the integer 0 (c0 = 1) by the same route as pai_encrypt_dev takes for these N elements, this
// obfuscator and this index_base; then one k_obf_mul. Out of place r^n goes straight into d_out; in place the call walks
// slices of obf_chunk elements through a buffer of its own (not ensure_work's: the encrypt chains reallocate that one
// for their intermediates while r^n is being produced).
int pai_obfuscate_dev(pai_ctx* c, const uint32_t* d_ct, size_t N, int obf_mode, const uint32_t* d_r_words,
                      size_t r_stride_words, size_t r_words, const uint8_t* rng_key32, uint64_t index_base,
                      uint32_t* d_out, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  if (N == 0) return 0;
  if (!d_ct || !d_out) return fail(PAI_ERR_ARG, "pai_obfuscate_dev: bad arguments");
  if (obf_mode != PAI_OBF_GIVEN && obf_mode != PAI_OBF_RNG && obf_mode != PAI_OBF_POOL)
    return fail(PAI_ERR_ARG, "pai_obfuscate_dev: obf_mode must be PAI_OBF_GIVEN, PAI_OBF_RNG or PAI_OBF_POOL");
  if (obf_mode == PAI_OBF_GIVEN && (!d_r_words || r_words == 0 || r_words > (size_t)c->ct_words))
    return fail(PAI_ERR_ARG, "pai_obfuscate_dev: r must be given with 0 < r_words <= ct_words");
  if (obf_mode == PAI_OBF_RNG && !rng_key32) return fail(PAI_ERR_ARG, "pai_obfuscate_dev: rng key required");
  const size_t W = c->ct_words;
  const bool in_place = d_out == d_ct;
  if (!in_place && d_out < d_ct + N * W && d_ct < d_out + N * W)
    return fail(PAI_ERR_ARG, "pai_obfuscate_dev: d_out must be d_ct or not overlap it");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  if (obf_mode == PAI_OBF_POOL) return pool_obfuscate_dev(c, d_ct, N, d_out, st);
  const size_t CH = in_place ? std::min(N, (size_t)c->obf_chunk) : N;
  const size_t rn_bytes = in_place ? align16(CH * W * 4) : 0, x_bytes = align16(CH * 8), e_bytes = align16(CH * 4);
  int rc = ensure_buf(&c->d_obf, &c->obf_bytes, rn_bytes + x_bytes + 2 * e_bytes);
  if (rc) return rc;
  uint32_t* rn = (uint32_t*)c->d_obf;
  int64_t* zeros = (int64_t*)((char*)c->d_obf + rn_bytes);
  int32_t* ex = (int32_t*)((char*)zeros + x_bytes);
  int32_t* status = (int32_t*)((char*)ex + e_bytes);
  HIPCHK(hipMemsetAsync(zeros, 0, CH * 8, st));
  ObfCall oc(c, obf_mode, (long long)N);
  for (size_t off = 0; off < N; off += CH) {
    const size_t n = std::min(CH, N - off);
    uint32_t* s = in_place ? rn : d_out + off * W;
    if ((rc = encrypt_dev(c, PAI_I64, zeros, n, PAI_EXP_AUTO, 0, obf_mode,
                          d_r_words ? d_r_words + off * r_stride_words : nullptr, r_stride_words, r_words, rng_key32,
                          index_base + off, s, ex, status, st)))
      return rc;
    if ((rc = launch_obf_mul(c, d_ct + off * W, s, d_out + off * W, (long long)n, st))) return rc;
  }
  return 0;
}

// ------------------------------------------------------------------ obfuscator pool (kernels_pool.hpp)
// A FIFO ring of ready r^n owned by the context. Fills and puts append at (head + ready) % cap, takes advance head; both
// move under the context's mutex when the call enqueues its work, and the device work of successive calls is ordered by
// the context's tail event, so a fill is complete before the take that follows it, on any stream.

// Waits for the context's queued device work, then frees the ring (re-keying, pai_pool_reserve)
static void pool_drop(pai_ctx* c) {
  pai_ctx::Pool& pl = c->pool;
  if (!pl.rows) return;
  if (c->tail_ev) (void)hipEventSynchronize(c->tail_ev);
  (void)hipFree(pl.rows);
  pl.rows = nullptr;
  pl.cap = pl.head = pl.ready = 0;
}

// The constants of the pool kernels: they depend on n alone and stay with the context
static int pool_consts(pai_ctx* c) {
  pai_ctx::Pool& pl = c->pool;
  if (pl.consts) return 0;
  const int S = c->S_e;
  const size_t Rbits = (size_t)LB * S;
  const HBig nneg = sub(pow2(Rbits), c->n);
  int rc;
  if ((rc = upload_to(c->allocs, nneg.limbs(S, LB), &pl.d_nneg)) ||
      (rc = upload_to(c->allocs, mul_pow2_mod(HBig(1), 2 * Rbits, c->n).limbs(S, LB), &pl.d_R2n)) ||
      (rc = upload_to(c->allocs, mul_pow2_mod(HBig(1), 2 * Rbits + 3 * LB, c->n).limbs(S, LB), &pl.d_R2n84)))
    return rc;
  pl.nprime = mont_prime(c->n, LB);
  pl.dprime = mont_prime(nneg, LB);
  pl.row_words = 2 * c->pt_words;
  pl.consts = true;
  return 0;
}

static PoolRing pool_ring(const pai_ctx* c, size_t first) {
  const pai_ctx::Pool& pl = c->pool;
  return PoolRing{pl.rows, (long long)pl.cap, (long long)first, pl.row_words, c->pt_words};
}

static int pool_grid(pai_ctx* c, int which, long long n) {
  int occ = 1;
  if (pool_occupancy(c->tpi_e, which, &occ)) return 0;
  const int gpb = BLOCK / c->tpi_e;
  return (int)std::max<long long>(1, std::min<long long>((n + gpb - 1) / gpb, (long long)occ * c->cus));
}

static int pool_check_take(pai_ctx* c, size_t N, const char* who) {
  const pai_ctx::Pool& pl = c->pool;
  if (!pl.rows) return fail(PAI_ERR_ARG, std::string(who) + ": PAI_OBF_POOL without a pool (pai_pool_reserve)");
  if (N > pl.ready)
    return fail(PAI_ERR_ARG, std::string(who) + ": the call takes " + std::to_string(N) + " obfuscators, the pool holds " +
                                 std::to_string(pl.ready));
  return 0;
}

// The head moves here, when the call is about to enqueue its work: whatever happens afterwards, these entries are spent
static size_t pool_advance(pai_ctx* c, size_t N) {
  pai_ctx::Pool& pl = c->pool;
  const size_t first = pl.head;
  pl.head = (pl.head + N) % pl.cap;
  pl.ready -= N;
  pl.taken += N;
  return first;
}

static int pool_check_room(pai_ctx* c, size_t count, const char* who) {
  const pai_ctx::Pool& pl = c->pool;
  if (!pl.rows) return fail(PAI_ERR_ARG, std::string(who) + ": no pool (pai_pool_reserve)");
  if (count > pl.cap - pl.ready)
    return fail(PAI_ERR_ARG, std::string(who) + ": " + std::to_string(count) + " entries do not fit the " +
                                 std::to_string(pl.cap - pl.ready) + " free of " + std::to_string(pl.cap));
  return 0;
}

// plain rho [n][W] -> the n ring rows behind the ready ones, which they join
static int pool_append(pai_ctx* c, const uint32_t* d_rho, size_t n, hipStream_t st) {
  pai_ctx::Pool& pl = c->pool;
  PoolSplitParams p{};
  p.rho = d_rho;
  p.ring = pool_ring(c, (pl.head + pl.ready) % pl.cap);
  p.n = (long long)n;
  p.nl = c->d_nl;
  p.nneg = pl.d_nneg;
  p.R2n = pl.d_R2n;
  p.R2n84 = pl.d_R2n84;
  p.nprime = pl.nprime;
  p.dprime = pl.dprime;
  p.ct_words = c->ct_words;
  const int grid = pool_grid(c, 2, p.n);
  if (!grid) return fail(PAI_ERR_KEY, "unsupported group size");
  HIPCHK(pool_split_launch(c->tpi_e, p, grid, st));
  pl.ready += n;
  return 0;
}

static PoolEncParams pool_enc_params(pai_ctx* c, size_t first, size_t N, uint32_t* d_ct) {
  PoolEncParams p{};
  p.ring = pool_ring(c, first);
  p.dst.ct = d_ct;
  p.dst.ct_words = c->ct_words;
  p.n = (long long)N;
  p.nl = c->d_nl;
  p.nprime = c->pool.nprime;
  return p;
}

// rows first .. first + N (wrapping) -> plain rho words
static int pool_join(pai_ctx* c, size_t first, size_t N, uint32_t* d_rho, hipStream_t st) {
  const PoolEncParams p = pool_enc_params(c, first, N, d_rho);
  const int grid = pool_grid(c, 1, p.n);
  if (!grid) return fail(PAI_ERR_KEY, "unsupported group size");
  HIPCHK(pool_join_launch(c->tpi_e, p, grid, st));
  return 0;
}

// pai_encrypt_dev with PAI_OBF_POOL below its argument checks: k_pool_enc, or (PAI_OPT_POOL_FUSED = 0) the kernels already
// pinned to the reference: k_pool_join, the PAI_OBF_NONE encryption, k_obf_mul
static int pool_encrypt_dev(pai_ctx* c, int dtype, const void* d_x, size_t N, int exp_mode, int32_t fixed_exp,
                            uint32_t* d_ct, int32_t* d_exp, int32_t* d_status, hipStream_t st) {
  int rc = pool_check_take(c, N, "pai_encrypt_dev");
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  if (!c->pool.fused && (rc = ensure_buf(&c->pool.d_rho, &c->pool.rho_bytes, N * c->ct_words * 4))) return rc;
  const size_t first = pool_advance(c, N);
  if (c->pool.fused) {
    PoolEncParams p = pool_enc_params(c, first, N, d_ct);
    p.src = EncPlain{d_x, dtype, exp_mode, fixed_exp};
    p.dst.exp = d_exp;
    p.dst.status = d_status;
    const int grid = pool_grid(c, 0, p.n);
    if (!grid) return fail(PAI_ERR_KEY, "unsupported group size");
    stage_reset(c);
    stage_mark(c, 0, st);
    HIPCHK(pool_enc_launch(c->tpi_e, p, grid, st));
    stage_mark(c, 1, st);
    return 0;
  }
  uint32_t* rho = (uint32_t*)c->pool.d_rho;
  if ((rc = pool_join(c, first, N, rho, st))) return rc;
  if ((rc = encrypt_dev(c, dtype, d_x, N, exp_mode, fixed_exp, PAI_OBF_NONE, nullptr, 0, 0, nullptr, 0, d_ct, d_exp,
                        d_status, st)))
    return rc;
  return launch_obf_mul(c, d_ct, rho, d_ct, (long long)N, st);
}

// pai_obfuscate_dev with PAI_OBF_POOL: the pooled rho joined straight into d_out (out of place) or, slice by slice, into
// the buffer the in-place call keeps its r^n in; then k_obf_mul
static int pool_obfuscate_dev(pai_ctx* c, const uint32_t* d_ct, size_t N, uint32_t* d_out, hipStream_t st) {
  int rc = pool_check_take(c, N, "pai_obfuscate_dev");
  if (rc) return rc;
  const size_t W = c->ct_words;
  const bool in_place = d_out == d_ct;
  const size_t CH = in_place ? std::min(N, (size_t)c->obf_chunk) : N;
  if (in_place && (rc = ensure_buf(&c->d_obf, &c->obf_bytes, align16(CH * W * 4)))) return rc;
  const size_t first = pool_advance(c, N);
  for (size_t off = 0; off < N; off += CH) {
    const size_t n = std::min(CH, N - off);
    uint32_t* s = in_place ? (uint32_t*)c->d_obf : d_out + off * W;
    if ((rc = pool_join(c, (first + off) % c->pool.cap, n, s, st))) return rc;
    if ((rc = launch_obf_mul(c, d_ct + off * W, s, d_out + off * W, (long long)n, st))) return rc;
  }
  return 0;
}

int pai_pool_reserve(pai_ctx* c, size_t capacity) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  HIPCHK(hipSetDevice(c->device));
  pool_drop(c);
  if (capacity == 0) return 0;
  int rc = pool_consts(c);
  if (rc) return rc;
  void* rows = nullptr;
  HIPCHK(dev_malloc(&rows, capacity * c->pool.row_words * 4));
  c->pool.rows = (uint32_t*)rows;
  c->pool.cap = capacity;
  return 0;
}

int pai_pool_info(pai_ctx* c, uint64_t* capacity, uint64_t* ready, uint64_t* taken_total) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (capacity) *capacity = c->pool.cap;
  if (ready) *ready = c->pool.ready;
  if (taken_total) *taken_total = c->pool.taken;
  return 0;
}

int pai_pool_put_dev(pai_ctx* c, const uint32_t* d_rho, size_t count, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  if (count == 0) return 0;
  if (!d_rho) return fail(PAI_ERR_ARG, "pai_pool_put_dev: null buffer");
  const int rc = pool_check_room(c, count, "pai_pool_put_dev");
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  return pool_append(c, d_rho, count, (hipStream_t)stream);
}

// Entry j is what pai_encrypt_dev writes for int64 zero at global index index_base + j: the encryption runs by that
// call's route into a slice buffer (the one pai_obfuscate_dev's in-place call keeps), one sampler decision for all
// `count` entries (ObfCall), and k_pool_split moves each slice into the ring
int pai_pool_fill_dev(pai_ctx* c, size_t count, int obf_mode, const uint32_t* d_r_words, size_t r_stride_words,
                      size_t r_words, const uint8_t* rng_key32, uint64_t index_base, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  if (obf_mode != PAI_OBF_GIVEN && obf_mode != PAI_OBF_RNG)
    return fail(PAI_ERR_ARG, "pai_pool_fill_dev: obf_mode must be PAI_OBF_GIVEN or PAI_OBF_RNG");
  if (obf_mode == PAI_OBF_GIVEN && (!d_r_words || r_words == 0 || r_words > (size_t)c->ct_words))
    return fail(PAI_ERR_ARG, "pai_pool_fill_dev: r must be given with 0 < r_words <= ct_words");
  if (obf_mode == PAI_OBF_RNG && !rng_key32) return fail(PAI_ERR_ARG, "pai_pool_fill_dev: rng key required");
  if (count == 0) return 0;
  int rc = pool_check_room(c, count, "pai_pool_fill_dev");
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t W = c->ct_words, CH = std::min(count, (size_t)c->obf_chunk);
  const size_t rn_bytes = align16(CH * W * 4), x_bytes = align16(CH * 8), e_bytes = align16(CH * 4);
  if ((rc = ensure_buf(&c->d_obf, &c->obf_bytes, rn_bytes + x_bytes + 2 * e_bytes))) return rc;
  uint32_t* rn = (uint32_t*)c->d_obf;
  int64_t* zeros = (int64_t*)((char*)c->d_obf + rn_bytes);
  int32_t* ex = (int32_t*)((char*)zeros + x_bytes);
  int32_t* status = (int32_t*)((char*)ex + e_bytes);
  HIPCHK(hipMemsetAsync(zeros, 0, CH * 8, st));
  ObfCall oc(c, obf_mode, (long long)count);
  for (size_t off = 0; off < count; off += CH) {
    const size_t n = std::min(CH, count - off);
    if ((rc = encrypt_dev(c, PAI_I64, zeros, n, PAI_EXP_AUTO, 0, obf_mode,
                          d_r_words ? d_r_words + off * r_stride_words : nullptr, r_stride_words, r_words, rng_key32,
                          index_base + off, rn, ex, status, st)))
      return rc;
    if ((rc = pool_append(c, rn, n, st))) return rc;
  }
  return 0;
}

template <int TPI>
static int launch_add(pai_ctx* c, AddParams& p, hipStream_t st) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  const size_t lds = (size_t)GPB * S * 4;
  const int grid = grid_for(c, k_add<TPI>, lds, p.n, GPB);
  hipLaunchKernelGGL(k_add<TPI>, dim3(grid), dim3(BLOCK), lds, st, p);
  HIPCHK(hipGetLastError());
  return 0;
}

// k-way add of p.k <= ADD_KMAX operands per instance: schedule sort (k_add_plan, k_add_scan,
// k_add_scatter) then the Horner product k_add (kernels.hpp).
static int run_add(pai_ctx* c, AddParams p, hipStream_t st) {
  if (p.n <= 0) return 0;
  const size_t nb_bucket = align16((size_t)p.n * 2), nb_perm = align16((size_t)p.n * 4);
  int rc = ensure_buf(&c->d_addplan, &c->addplan_bytes, nb_bucket + nb_perm + ADD_TMAX * 4);
  if (rc) return rc;
  uint16_t* bucket = (uint16_t*)c->d_addplan;
  int* perm = (int*)((char*)c->d_addplan + nb_bucket);
  unsigned* hist = (unsigned*)((char*)c->d_addplan + nb_bucket + nb_perm);
  p.N = c->d_N;
  p.RS = c->d_RS;
  p.mprime = c->mprime_N;
  p.ct_words = c->ct_words;
  p.perm = nullptr;
  const int g = (int)std::max<long long>(1, std::min<long long>((p.n + 255) / 256, 8ll * c->cus));
  HIPCHK(hipMemsetAsync(hist, 0, ADD_TMAX * 4, st));
  hipLaunchKernelGGL(k_add_plan<0>, dim3(g), dim3(256), 0, st, p, bucket, hist);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_add_scan<0>, dim3(1), dim3(ADD_TMAX), 0, st, hist, p.gate);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_add_scatter<0>, dim3(g), dim3(256), 0, st, (long long)p.n, (const uint16_t*)bucket, hist, perm,
                     p.gate);
  HIPCHK(hipGetLastError());
  p.perm = perm;
  switch (c->tpi_e) {
    case 2: return launch_add<2>(c, p, st);
    case 4: return launch_add<4>(c, p, st);
    case 8: return launch_add<8>(c, p, st);
  }
  return fail(PAI_ERR_KEY, "unsupported group size");
}

static AddParams add_params(const uint32_t* cts, const int32_t* exps, int k, long long N, uint32_t* out, int32_t* out_exp,
                            const long long* gidx = nullptr) {
  AddParams p{};
  p.cts = cts;
  p.exps = exps;
  p.k = k;
  p.out = out;
  p.out_exp = out_exp;
  p.n = N;
  p.gidx = gidx;
  return p;
}

static int add_dev(pai_ctx* c, const uint32_t* cts, const int32_t* exps, int k, long long N, uint32_t* out,
                   int32_t* out_exp, hipStream_t st);

int pai_add_dev(pai_ctx* c, const uint32_t* d_cts, const int32_t* d_exps, int k, size_t N, uint32_t* d_out,
                int32_t* d_exp_out, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  if (N == 0) return 0;
  if (k < 1 || !d_cts || !d_exps || !d_out || !d_exp_out) return fail(PAI_ERR_ARG, "pai_add_dev: bad arguments");
  HIPCHK(hipSetDevice(c->device));
  return add_dev(c, d_cts, d_exps, k, (long long)N, d_out, d_exp_out, (hipStream_t)stream);
}

template <int TPI>
static int launch_decrypt(pai_ctx* c, DecParams& p, hipStream_t st) {
  constexpr int S = TPI * L;
  constexpr int EPB = BLOCK / (2 * TPI);
  const size_t lds = (size_t)EPB * 4 * S * 4;
  const int grid = grid_for(c, k_decrypt<TPI>, lds, p.n, EPB);
  int rc = ensure_scratch(c, (size_t)grid * EPB * 2 * TABLE_FIX * S * 4);
  if (rc) return rc;
  p.scratch = (uint32_t*)c->d_scratch;
  hipLaunchKernelGGL(k_decrypt<TPI>, dim3(grid), dim3(BLOCK), lds, st, p);
  HIPCHK(hipGetLastError());
  return 0;
}

// pair decryption (kernels_pair.hpp, engine_pair.hip), in chunks of CRT_CHUNK elements
// The pair kernels' final stage over elements [off, off + n) from the pairs in xw ([2][2S][n])
static DecPairFinParams dec_pair_fin_params(pai_ctx* c, const DecParams& d, uint32_t* xw, long long off, long long n) {
  DecPairFinParams f{};
  f.halves = c->d_decp_halves;
  f.n = n;
  f.xh = xw;
  f.exp = d.exp + off;
  f.p = c->d_dec_p;
  f.q = c->d_dec_q;
  f.qinvR = c->d_dec_qinvR;
  f.pprime = c->dec_pprime;
  f.nlimb = c->d_decp_nl;
  f.maxint = c->d_decp_maxint;
  f.val = d.val + off;
  f.mant = d.mant ? d.mant + off : nullptr;
  f.status = d.status + off;
  f.raw = d.raw ? d.raw + (size_t)off * c->pt_words : nullptr;
  f.pt_words = c->pt_words;
  return f;
}

// A call of at most crtw_max ciphertexts: c^(p_h - 1) mod p_h^2 on 16-lane rows (k_dec_w, kernels_crtw.hpp) into
// the pairs k_dec_fin_pair takes; stage times: k_dec_w, k_dec_fin_pair.
static int launch_decw(pai_ctx* c, const DecParams& d, hipStream_t st) {
  const long long N = d.n;
  const int S = c->crt_sa;
  int rc = ensure_work(c, (size_t)4 * S * N * 4);
  if (rc) return rc;
  uint32_t* xw = (uint32_t*)c->d_work;
  crtw::DecParams p{c->d_decw, c->d_crt_a, N, d.ct, c->ct_words, c->decw_kchunks, xw};
  stage_mark(c, 0, st);
  HIPCHK(decw_launch(S, p, st));
  stage_mark(c, 1, st);
  const DecPairFinParams f = dec_pair_fin_params(c, d, xw, 0, N);
  HIPCHK(dec_pair_launch_fin(S, f, (int)std::min<long long>((N + LANE_BLOCK - 1) / LANE_BLOCK, 4ll * c->cus), st));
  stage_mark(c, 2, st);
  return 0;
}

static int launch_dec_pair(pai_ctx* c, const DecParams& d, hipStream_t st) {
  const long long N = d.n;
  if (N <= c->crtw_max && c->d_decw) return launch_decw(c, d, st);
  const long long chunk = std::min(N, CRT_CHUNK);
  const int S = c->crt_sa;
  DecLaneGeom g;
  if (dec_pair_geometry(S, c->cus, chunk, &g, c->decf)) return fail(PAI_ERR_KEY, "pair decrypt: unsupported size");
  int rc = ensure_scratch(c, g.scratch_bytes);
  if (rc) return rc;
  if ((rc = ensure_work(c, (size_t)4 * S * chunk * 4))) return rc;
  for (long long off = 0; off < N; off += chunk) {
    const long long n = std::min(chunk, N - off);
    hipEvent_t* ev = stage_chunk(c);
    if (ev) c->nev = 4;
    uint32_t* xw = (uint32_t*)c->d_work;   // [2][2S][n]: c~, then x_h in place
    DecPairPreParams pre{c->d_decp_halves, n, d.ct + (size_t)off * c->ct_words, c->ct_words, c->decp_kchunks, xw};
    CrtParams pw{};
    pw.halves = c->d_decp_pow;
    pw.n = n;
    pw.yin = xw;
    pw.out = xw;
    pw.scratch = (uint32_t*)c->d_scratch;
    const DecPairFinParams f = dec_pair_fin_params(c, d, xw, off, n);
    HIPCHK(dec_pair_launch(S, pre, pw, f, g, st, ev, c->decf));
  }
  return 0;
}

// 4096-bit split-pair decryption (kernels_dec4.hpp, engine_dec4.hip), in chunks of CRT_CHUNK elements
// A 4096-bit call of at most crtw_max ciphertexts: c^(p_h - 1) mod p_h^2 on rows (k_dec_w<74, 148>) into the pairs
// k_dec4_L takes, then k_dec4_L and k_dec4_fin; stage times: k_dec_w, k_dec4_L + k_dec4_fin.
static int launch_decw4(pai_ctx* c, const DecParams& d, hipStream_t st) {
  const long long N = d.n;
  Dec4Geom g;
  dec4_geometry(c->cus, N, &g);
  const size_t xbytes = (size_t)2 * 2 * D4_S * 4, mbytes = (size_t)2 * D4_S * 4;   // per element
  int rc = ensure_work(c, (xbytes + mbytes) * N);
  if (rc) return rc;
  Dec4Params p{};
  p.halves = c->d_dec4_halves;
  p.n = N;
  p.ct = d.ct;
  p.ct_words = c->ct_words;
  p.kchunks = c->dec4_kchunks;
  p.x = (uint32_t*)c->d_work;
  p.mh = (uint32_t*)((char*)c->d_work + xbytes * N);
  p.scratch = (uint32_t*)c->d_scratch;
  crtw::DecParams w{c->d_decw, c->d_crt_a, N, d.ct, c->ct_words, c->decw_kchunks, p.x};
  stage_mark(c, 0, st);
  HIPCHK(decw_launch(c->rows_sa, w, st));
  stage_mark(c, 1, st);
  HIPCHK(dec4_launch_tail(p, d, g, st));
  stage_mark(c, 2, st);
  return 0;
}

static int launch_dec4(pai_ctx* c, const DecParams& d, hipStream_t st) {
  const long long N = d.n;
  if (N <= c->crtw_max && c->rows_sa && c->d_decw) return launch_decw4(c, d, st);
  const long long chunk = std::min(N, CRT_CHUNK);
  Dec4Geom g;
  dec4_geometry(c->cus, chunk, &g);
  int rc = ensure_scratch(c, g.scratch_bytes);
  if (rc) return rc;
  const size_t xbytes = (size_t)2 * 2 * D4_S * 4, mbytes = (size_t)2 * D4_S * 4;   // per element
  if ((rc = ensure_work(c, (xbytes + mbytes) * chunk))) return rc;
  for (long long off = 0; off < N; off += chunk) {
    const long long n = std::min(chunk, N - off);
    hipEvent_t* ev = stage_chunk(c);
    if (ev) c->nev = 4;
    Dec4Params p{};
    p.halves = c->d_dec4_halves;
    p.n = n;
    p.ct = d.ct + (size_t)off * c->ct_words;
    p.ct_words = c->ct_words;
    p.kchunks = c->dec4_kchunks;
    p.x = (uint32_t*)c->d_work;
    p.mh = (uint32_t*)((char*)c->d_work + xbytes * chunk);
    p.scratch = (uint32_t*)c->d_scratch;
    DecParams f = d;
    f.ct += (size_t)off * c->ct_words;
    f.exp += off;
    f.n = n;
    f.val += off;
    if (f.mant) f.mant += off;
    f.status += off;
    if (f.raw) f.raw += (size_t)off * c->pt_words;
    HIPCHK(dec4_launch(p, f, g, st, ev));
  }
  return 0;
}

int pai_decrypt_dev(pai_ctx* c, const uint32_t* d_ct, const int32_t* d_exp, size_t N, double* d_val, int64_t* d_mant,
                    int32_t* d_status, uint32_t* d_raw, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  if (!c->has_priv) return fail(PAI_ERR_NOPRIV, "pai_decrypt: context has no private key");
  if (N == 0) return 0;
  if (!d_ct || !d_exp || !d_val || !d_status) return fail(PAI_ERR_ARG, "pai_decrypt_dev: bad arguments");
  HIPCHK(hipSetDevice(c->device));
  stage_reset(c);
  DecParams p{};
  p.ct = d_ct;
  p.exp = d_exp;
  p.n = (long long)N;
  p.val = d_val;
  p.mant = d_mant;
  p.status = d_status;
  p.raw = d_raw;
  p.halves = c->d_halves;
  p.qinvR = c->d_qinvR;
  p.nlimb = c->d_nlimb;
  p.qRn = c->d_qRn;
  p.maxint = c->d_maxint;
  p.nprime = c->nprime_d;
  p.nwin = c->nwin;
  p.ct_words = c->ct_words;
  p.pt_words = c->pt_words;
  p.n_limbs = c->n_limbs;
  hipStream_t st = (hipStream_t)stream;
  if (c->dec_pair_ok && c->dec_lane_enabled) return launch_dec_pair(c, p, st);
  if (c->dec4_ok && c->dec_lane_enabled) return launch_dec4(c, p, st);
  switch (c->tpi_d) {
    case 1: return launch_decrypt<1>(c, p, st);
    case 2: return launch_decrypt<2>(c, p, st);
    case 4: return launch_decrypt<4>(c, p, st);
  }
  return fail(PAI_ERR_KEY, "unsupported group size");
}

// ------------------------------------------------------------------ packed plaintexts (kernels_pack.hpp)
static int pack_layout(const pai_ctx* c, const pai_pack_layout* l, PackLayout* out) {
  if (!l) return fail(PAI_ERR_ARG, "packed layout: null");
  if (l->slot_bits < 16 || l->slot_bits > 64 || l->slot_bits % 8)
    return fail(PAI_ERR_ARG, "packed layout: slot_bits must be a multiple of 8 in [16, 64]");
  if (l->value_bits < 2 || l->value_bits > l->slot_bits)
    return fail(PAI_ERR_ARG, "packed layout: value_bits must be in [2, slot_bits]");
  if (l->slots < 1 || l->slots > (c->nb - 2) / l->slot_bits)
    return fail(PAI_ERR_ARG, "packed layout: slots must be in [1, (key_bits - 2) / slot_bits]");
  *out = PackLayout{l->slot_bits, l->value_bits, l->exponent, l->slots};
  return 0;
}

int pai_pack_max_slots(const pai_ctx* c, int slot_bits, int* slots) {
  if (!c || !slots) return fail(PAI_ERR_ARG, "pai_pack_max_slots: null argument");
  if (slot_bits < 16 || slot_bits > 64 || slot_bits % 8)
    return fail(PAI_ERR_ARG, "pai_pack_max_slots: slot_bits must be a multiple of 8 in [16, 64]");
  *slots = (c->nb - 2) / slot_bits;
  return 0;
}

// E0 = the encryption of ceil(N / slots) int64 zeros goes straight into d_ct by pai_encrypt_dev's own route (skipped for
// PAI_OBF_NONE), then one k_pack_mul forms c0 of every ciphertext and multiplies in place.
int pai_encrypt_packed_dev(pai_ctx* c, int dtype, const void* d_x, size_t N, const pai_pack_layout* layout, int obf_mode,
                           const uint32_t* d_r_words, size_t r_stride_words, size_t r_words, const uint8_t* rng_key32,
                           uint64_t index_base, uint32_t* d_ct, int32_t* d_status, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  PackLayout lay;
  int rc = pack_layout(c, layout, &lay);
  if (rc) return rc;
  if (N == 0) return 0;
  if (dtype < 0 || dtype > 2 || !d_x || !d_ct) return fail(PAI_ERR_ARG, "pai_encrypt_packed_dev: bad arguments");
  if (obf_mode == PAI_OBF_GIVEN && (!d_r_words || r_words == 0 || r_words > (size_t)c->ct_words))
    return fail(PAI_ERR_ARG, "pai_encrypt_packed_dev: r must be given with 0 < r_words <= ct_words");
  if (obf_mode == PAI_OBF_RNG && !rng_key32) return fail(PAI_ERR_ARG, "pai_encrypt_packed_dev: rng key required");
  if (obf_mode < 0 || obf_mode > 2) return fail(PAI_ERR_ARG, "pai_encrypt_packed_dev: bad obf_mode");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t C = (N + lay.k - 1) / lay.k;
  if (obf_mode != PAI_OBF_NONE) {
    const size_t x_bytes = align16(C * 8), e_bytes = align16(C * 4);
    if ((rc = ensure_buf(&c->d_pack, &c->pack_bytes, x_bytes + 2 * e_bytes))) return rc;
    int64_t* zeros = (int64_t*)c->d_pack;
    int32_t* ex = (int32_t*)((char*)zeros + x_bytes);
    int32_t* status = (int32_t*)((char*)ex + e_bytes);
    HIPCHK(hipMemsetAsync(zeros, 0, C * 8, st));
    if ((rc = encrypt_dev(c, PAI_I64, zeros, C, PAI_EXP_AUTO, 0, obf_mode, d_r_words, r_stride_words, r_words, rng_key32,
                          index_base, d_ct, ex, status, st)))
      return rc;
  }
  int occ = 1;
  if (pack_occupancy(c->tpi_e, &occ)) return fail(PAI_ERR_KEY, "unsupported group size");
  const int gpb = BLOCK / c->tpi_e;
  PackMulParams p{};
  p.x = d_x;
  p.dtype = dtype;
  p.nvals = (long long)N;
  p.lay = lay;
  p.obf = obf_mode;
  p.ct = d_ct;
  p.status = d_status;
  p.n = (long long)C;
  p.N = c->d_N;
  p.R2 = c->d_R2;
  p.nl = c->d_nl;
  p.mprime = c->mprime_N;
  p.ct_words = c->ct_words;
  p.n_limbs = (c->nb + LB - 1) / LB;
  p.m_limbs = (lay.k * lay.sb - 1 + LB - 1) / LB;   // |M| < 2^(k sb - 1)
  const int grid = (int)std::max<long long>(1, std::min<long long>((p.n + gpb - 1) / gpb, (long long)occ * c->cus));
  HIPCHK(pack_launch(c->tpi_e, p, grid, st));
  return 0;
}

// The decrypt chain pai_decrypt_dev picks for these ciphertexts, with the raw plaintexts requested, then k_unpack.
int pai_decrypt_packed_dev(pai_ctx* c, const uint32_t* d_ct, const pai_pack_layout* layout, size_t N, double* d_val,
                           int64_t* d_mant, int32_t* d_status, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  PackLayout lay;
  int rc = pack_layout(c, layout, &lay);
  if (rc) return rc;
  if (!c->has_priv) return fail(PAI_ERR_NOPRIV, "pai_decrypt_packed: context has no private key");
  if (N == 0) return 0;
  if (!d_ct || !d_val || !d_status) return fail(PAI_ERR_ARG, "pai_decrypt_packed_dev: bad arguments");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t C = (N + lay.k - 1) / lay.k, PW = c->pt_words;
  if (!c->d_pack_consts) {
    const HBig maxint = sub(div_small(c->n, 3), HBig(1));   // keypair.py:29
    std::vector<uint32_t> cs = c->n.words(PW);
    append(cs, maxint.words(PW));
    append(cs, sub(c->n, maxint).words(PW));
    if ((rc = upload_to(c->allocs, cs, &c->d_pack_consts))) return rc;
  }
  const size_t e_bytes = align16(C * 4), v_bytes = align16(C * 8), raw_bytes = align16(C * PW * 4);
  if ((rc = ensure_buf(&c->d_pack, &c->pack_bytes, 2 * e_bytes + v_bytes + raw_bytes))) return rc;
  double* val = (double*)c->d_pack;
  uint32_t* raw = (uint32_t*)((char*)val + v_bytes);
  int32_t* ex = (int32_t*)((char*)raw + raw_bytes);
  int32_t* status = (int32_t*)((char*)ex + e_bytes);
  HIPCHK(hipMemsetAsync(ex, 0, C * 4, st));
  if ((rc = pai_decrypt_dev(c, d_ct, ex, C, val, nullptr, status, raw, stream))) return rc;
  UnpackParams u{};
  u.raw = raw;
  u.n = (long long)C;
  u.nvals = (long long)N;
  u.lay = lay;
  u.val = d_val;
  u.mant = d_mant;
  u.status = d_status;
  u.consts = c->d_pack_consts;
  u.pt_words = (int)PW;
  const int grid = (int)std::max<long long>(1, std::min<long long>((u.n + UNPACK_CPB - 1) / UNPACK_CPB, 8ll * c->cus));
  HIPCHK(unpack_launch(u, grid, st));
  return 0;
}

// Largest output count that the automatic choice (PAI_OPT_FOLD_ROWS = 1) sends to the rows: the measured crossings of
// tools/fold_ab.py (include/flexpai.h), per size of n^2 in limbs.
static long long fold_rows_max(int k) {
  return k == 74 ? PAI_FOLD_ROWS_MAX_1024 : k == 148 ? PAI_FOLD_ROWS_MAX_2048 : k == 296 ? PAI_FOLD_ROWS_MAX_4096 : 0;
}

// A host-buffer fold decides rows or groups once, by the outputs of the whole call: its chunks run one after the other
// on one stream, so a call above the threshold gains nothing from chunks that happen to lie below it.
struct FoldCall {
  pai_ctx* c;
  FoldCall(pai_ctx* ctx, size_t outputs) : c(ctx) { c->fold_call_n = (long long)outputs; }
  ~FoldCall() { c->fold_call_n = 0; }
};

// One fold over p.n outputs: k_pack_fold_w on 16-lane rows for calls of few outputs, k_pack_fold on lane groups
// otherwise. No scratch, no inversion, nothing read back; the constants are filled here.
static int fold_run(pai_ctx* c, PackFoldParams& p, hipStream_t st) {
  p.N = c->d_N;
  p.R2 = c->d_R2;
  p.oneR = c->d_oneR;
  p.mprime = c->mprime_N;
  p.ct_words = c->ct_words;
  const long long total = c->fold_call_n ? c->fold_call_n : p.n;
  const bool rows = foldw_has(c->S_e) && (c->fold_rows == 2 || (c->fold_rows == 1 && total <= fold_rows_max(c->S_e)));
  if (rows) {
    HIPCHK(foldw_launch(c->S_e, p, st));
    c->fold_path = 2;
    return 0;
  }
  int occ = 1;
  if (fold_occupancy(c->tpi_e, &occ)) return fail(PAI_ERR_KEY, "unsupported group size");
  const int gpb = BLOCK / c->tpi_e;
  const int grid = (int)std::max<long long>(1, std::min<long long>((p.n + gpb - 1) / gpb, (long long)occ * c->cus));
  HIPCHK(fold_launch(c->tpi_e, p, grid, st));
  c->fold_path = 1;
  return 0;
}

// Packed ciphertexts folded into wider ones (include/flexpai.h pai_repack): k_pack_fold's walk with the stride s sb and
// no exponents. Every argument is checked before the launch.
int pai_repack_dev(pai_ctx* c, const uint32_t* d_ct, size_t N, const pai_pack_layout* in_layout, int group,
                   uint32_t* d_out, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  PackLayout lay;
  int rc = pack_layout(c, in_layout, &lay);
  if (rc) return rc;
  if (group < 1 || (long long)lay.k * group > (c->nb - 2) / lay.sb)
    return fail(PAI_ERR_ARG, "pai_repack: slots * group must be in [slots, (key_bits - 2) / slot_bits]");
  if (N == 0) return 0;
  if (!d_ct || !d_out) return fail(PAI_ERR_ARG, "pai_repack_dev: bad arguments");
  const size_t W = c->ct_words, C = (N + group - 1) / group;
  if (d_out < d_ct + N * W && d_ct < d_out + C * W)
    return fail(PAI_ERR_ARG, "pai_repack_dev: d_out must not overlap d_ct");
  HIPCHK(hipSetDevice(c->device));
  PackFoldParams p{};
  p.ct = d_ct;
  p.exp = nullptr;
  p.nvals = (long long)N;
  p.lay = PackLayout{lay.sb, lay.vb, lay.fexp, group};
  p.stride = lay.k * lay.sb;
  p.out = d_out;
  p.status = nullptr;
  p.n = (long long)C;
  return fold_run(c, p, (hipStream_t)stream);
}

// One fold over the ceil(N / slots) outputs.
int pai_pack_ciphertexts_dev(pai_ctx* c, const uint32_t* d_ct, const int32_t* d_exp, size_t N,
                             const pai_pack_layout* layout, uint32_t* d_out, int32_t* d_status, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  PackLayout lay;
  int rc = pack_layout(c, layout, &lay);
  if (rc) return rc;
  if (N == 0) return 0;
  if (!d_ct || !d_exp || !d_out) return fail(PAI_ERR_ARG, "pai_pack_ciphertexts_dev: bad arguments");
  const size_t W = c->ct_words, C = (N + lay.k - 1) / lay.k;
  if (d_out < d_ct + N * W && d_ct < d_out + C * W)
    return fail(PAI_ERR_ARG, "pai_pack_ciphertexts_dev: d_out must not overlap d_ct");
  HIPCHK(hipSetDevice(c->device));
  PackFoldParams p{};
  p.ct = d_ct;
  p.exp = d_exp;
  p.nvals = (long long)N;
  p.lay = lay;
  p.stride = lay.sb;
  p.out = d_out;
  p.status = d_status;
  p.n = (long long)C;
  return fold_run(c, p, (hipStream_t)stream);
}

// ------------------------------------------------------------------ host-buffer entry points
struct DevScope {
  std::vector<void*> ptrs;
  ~DevScope() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  template <typename T>
  T* alloc(size_t n) {
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) return nullptr;
    ptrs.push_back(p);
    return (T*)p;
  }
};

// ------------------------------------------------------------------ ciphertext x plaintext

static int inv_grid(pai_ctx* c, int tpi, long long nseg) {
  int occ = 1;
  if (mul_occupancy(tpi, &occ)) occ = 1;
  const int gpb = BLOCK / tpi;
  return (int)std::max<long long>(1, std::min<long long>((nseg + gpb - 1) / gpb, (long long)occ * c->cus));
}

// Batch inversion (Montgomery's trick, kernels_mul.hpp) of the flagged values of x [n][W] in place,
// on `st`. Segment products are reduced level by level to ONE value, inverted on the host (the only
// modular inversion mod n^2; gmpy_math.invert, gmpy_math.py:66-74), and expanded back down. The
// host step synchronises `st` once. Not invertible -> PAI_ERR_NOINV ("no inverse exists").
static int batch_invert(pai_ctx* c, uint32_t* x, const uint8_t* flag, long long n, hipStream_t st) {
  return batch_invert(c, x, flag, n, st, InvMod{c->tpi_e, c->ct_words, c->S_e, c->d_N, c->d_R2, c->d_oneR, c->mprime_N, &c->N});
}
static int batch_invert(pai_ctx* c, uint32_t* x, const uint8_t* flag, long long n, hipStream_t st, const InvMod& md) {
  const int S = md.S, W = md.W;
  // segment length per level: INV_SEG where there are values enough to fill the chip with segments, down to 4 on the
  // upper levels, whose few groups would otherwise walk chains of 64 dependent products (round 5: the 1M-value
  // inversion's levels above the first took ~22 of its 37 ms as 64-long chains over 16 k, 256 and 4 values)
  std::vector<long long> ns{n};
  std::vector<int> seg;
  do {
    seg.push_back((int)std::max<long long>(4, std::min<long long>(INV_SEG, ns.back() / 4096)));
    ns.push_back((ns.back() + seg.back() - 1) / seg.back());
  } while (ns.back() > 1);
  const int levels = (int)ns.size() - 1;
  std::vector<size_t> pre_off(levels), seg_off(levels);
  size_t off = 0;
  for (int l = 0; l < levels; ++l) {
    pre_off[l] = off;
    off = align16(off + (size_t)ns[l] * S * 4);
    seg_off[l] = off;
    off = align16(off + (size_t)ns[l + 1] * W * 4);
  }
  int rc = ensure_buf(&c->d_inv, &c->inv_bytes, off);
  if (rc) return rc;
  char* base = (char*)c->d_inv;
  auto params = [&](int l) {
    InvParams p{};
    p.x = l == 0 ? x : (uint32_t*)(base + seg_off[l - 1]);
    p.flag = l == 0 ? flag : nullptr;
    p.n = ns[l];
    p.pre = (uint32_t*)(base + pre_off[l]);
    p.seg = (uint32_t*)(base + seg_off[l]);
    p.N = md.N;
    p.R2 = md.R2;
    p.oneR = md.oneR;
    p.mprime = md.mprime;
    p.ct_words = W;
    p.seg_len = seg[l];
    return p;
  };
  for (int l = 0; l < levels; ++l) HIPCHK(inv_launch(md.tpi, true, params(l), inv_grid(c, md.tpi, ns[l + 1]), st));
  uint32_t* top = (uint32_t*)(base + seg_off[levels - 1]);
  c->inv_host.assign(W, 0);
  HIPCHK(hipMemcpyAsync(c->inv_host.data(), top, (size_t)W * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HBig v;
  v.w = c->inv_host;
  v.trim();
  HBig inv = inv_mod(v, *md.mod);
  if (inv.is_zero()) return fail(PAI_ERR_NOINV, "invert() no inverse exists");
  c->inv_host = inv.words(W);
  HIPCHK(hipMemcpyAsync(top, c->inv_host.data(), (size_t)W * 4, hipMemcpyHostToDevice, st));
  for (int l = levels - 1; l >= 0; --l) HIPCHK(inv_launch(md.tpi, false, params(l), inv_grid(c, md.tpi, ns[l + 1]), st));
  return 0;
}

// The public-key encryption's batch inversion (launch_pe) without blocking the caller: batch_invert's levels, but the top
// value is inverted by a host function queued on `st` (hipLaunchHostFunc: it runs when the stream reaches it, on the
// runtime's thread, touching only the pinned words) instead of after a hipStreamSynchronize, so pai_encrypt_dev stays
// asynchronous and capturable. An A_r that shares a factor with n (no inverse, probability ~2^-1023 for
// random r; r = 0, n, 5p given explicitly) sets *d_noinv = 1, and the kernels choose the chain on the device:
// k_pe_iota / k_pe_pow_f exit, the general k_pe_pow runs (kernels_pe.hpp, PeParams::noinv).
static void inv_top_host(void* u) {
  auto* a = (pai_ctx::AsyncInv*)u;
  try {
    HBig v;
    v.w.assign(a->pin, a->pin + a->W);
    v.trim();
    const HBig inv = inv_mod(v, a->mod);
    if (inv.is_zero()) {
      a->pin[a->W] = 1u;
      return;
    }
    const std::vector<uint32_t> w = inv.words(a->W);
    std::memcpy(a->pin, w.data(), (size_t)a->W * 4);
    a->pin[a->W] = 0u;
  } catch (...) {
    a->pin[a->W] = 1u;   // the general chain, same ciphertexts
  }
}

static int batch_invert_async(pai_ctx* c, uint32_t* x, long long n, hipStream_t st, const InvMod& md, uint32_t** d_noinv) {
  const int S = md.S, W = md.W;
  std::vector<long long> ns{n};
  std::vector<int> seg;
  do {
    seg.push_back((int)std::max<long long>(4, std::min<long long>(INV_SEG, ns.back() / 4096)));
    ns.push_back((ns.back() + seg.back() - 1) / seg.back());
  } while (ns.back() > 1);
  const int levels = (int)ns.size() - 1;
  std::vector<size_t> pre_off(levels), seg_off(levels);
  size_t off = 0;
  for (int l = 0; l < levels; ++l) {
    pre_off[l] = off;
    off = align16(off + (size_t)ns[l] * S * 4);
    seg_off[l] = off;
    off = align16(off + (size_t)ns[l + 1] * W * 4);
  }
  const size_t flag_off = off;
  off += 16;
  int rc = ensure_buf(&c->d_inv, &c->inv_bytes, off);
  if (rc) return rc;
  if (!c->inv_async || c->inv_async->W != W || !(c->inv_async->mod.w == md.mod->w)) {
    if (!c->inv_async) c->inv_async = new pai_ctx::AsyncInv;
    if (c->inv_async->pin && c->inv_async->W < W) {
      HIPCHK(hipStreamSynchronize(st));   // (once per context: a previous call's host function may still read it)
      (void)hipHostFree(c->inv_async->pin);
      c->inv_async->pin = nullptr;
    }
    if (!c->inv_async->pin) HIPCHK(hipHostMalloc((void**)&c->inv_async->pin, (size_t)(W + 4) * 4, hipHostMallocDefault));
    c->inv_async->W = W;
    c->inv_async->mod = *md.mod;
  }
  char* base = (char*)c->d_inv;
  auto params = [&](int l) {
    InvParams p{};
    p.x = l == 0 ? x : (uint32_t*)(base + seg_off[l - 1]);
    p.flag = nullptr;
    p.n = ns[l];
    p.pre = (uint32_t*)(base + pre_off[l]);
    p.seg = (uint32_t*)(base + seg_off[l]);
    p.N = md.N;
    p.R2 = md.R2;
    p.oneR = md.oneR;
    p.mprime = md.mprime;
    p.ct_words = W;
    p.seg_len = seg[l];
    return p;
  };
  for (int l = 0; l < levels; ++l) HIPCHK(inv_launch(md.tpi, true, params(l), inv_grid(c, md.tpi, ns[l + 1]), st));
  uint32_t* top = (uint32_t*)(base + seg_off[levels - 1]);
  uint32_t* flag = (uint32_t*)(base + flag_off);
  uint32_t* pin = c->inv_async->pin;
  HIPCHK(hipMemcpyAsync(pin, top, (size_t)W * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipLaunchHostFunc(st, inv_top_host, c->inv_async));
  HIPCHK(hipMemcpyAsync(top, pin, (size_t)W * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(flag, pin + W, 4, hipMemcpyHostToDevice, st));
  // (with no inverse the words copied back are the top value itself: the levels below produce values nobody reads)
  for (int l = levels - 1; l >= 0; --l) HIPCHK(inv_launch(md.tpi, false, params(l), inv_grid(c, md.tpi, ns[l + 1]), st));
  *d_noinv = flag;
  return 0;
}

// k_mul over n terms (p: index maps, scalars; outputs set by the caller)
static int launch_mul(pai_ctx* c, MulParams& p, hipStream_t st) {
  int occ = 1;
  if (mul_occupancy(c->tpi_e, &occ)) return fail(PAI_ERR_KEY, "unsupported group size");
  const int gpb = BLOCK / c->tpi_e;
  const int grid = (int)std::max<long long>(1, std::min<long long>((p.n + gpb - 1) / gpb, (long long)occ * c->cus));
  int rc = ensure_scratch(c, (size_t)grid * BLOCK * TILE_WORDS_PER_LANE * 4);
  if (rc) return rc;
  p.N = c->d_N;
  p.R2 = c->d_R2;
  p.oneR = c->d_oneR;
  p.mprime = c->mprime_N;
  p.ct_words = c->ct_words;
  p.scratch = (uint32_t*)c->d_scratch;
  HIPCHK(mul_launch(c->tpi_e, p, grid, st));
  return 0;
}

// k consecutive [N][W] operand arrays; more than ADD_KMAX operands are summed in chunks of ADD_KMAX
// (the partial sums are exact ciphertexts, so the result is the same integer)
static int add_dev(pai_ctx* c, const uint32_t* cts, const int32_t* exps, int k, long long N, uint32_t* out,
                   int32_t* out_exp, hipStream_t st) {
  if (k <= ADD_KMAX) return run_add(c, add_params(cts, exps, k, N, out, out_exp), st);
  const int parts = (k + ADD_KMAX - 1) / ADD_KMAX;
  const size_t W = c->ct_words;
  uint32_t* pc = nullptr;
  int32_t* pe = nullptr;
  HIPCHK(hipMallocAsync((void**)&pc, (size_t)parts * N * W * 4, st));
  HIPCHK(hipMallocAsync((void**)&pe, (size_t)parts * N * 4, st));
  int rc = 0;
  for (int q = 0; q < parts && !rc; ++q) {
    const int kq = std::min(ADD_KMAX, k - q * ADD_KMAX);
    rc = run_add(c, add_params(cts + (size_t)q * ADD_KMAX * N * W, exps + (size_t)q * ADD_KMAX * N, kq, N,
                               pc + (size_t)q * N * W, pe + (size_t)q * N), st);
  }
  if (!rc) rc = add_dev(c, pc, pe, parts, N, out, out_exp, st);
  (void)hipFreeAsync(pc, st);
  (void)hipFreeAsync(pe, st);
  return rc;
}

int pai_mul_dev(pai_ctx* c, const uint32_t* d_ct, const int32_t* d_exp, size_t N, int dtype, const void* d_x,
                size_t x_stride, uint32_t* d_out, int32_t* d_exp_out, int32_t* d_status, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  if (N == 0) return 0;
  if (!d_ct || !d_exp || !d_x || !d_out || !d_exp_out || dtype < 0 || dtype > 2 || x_stride > 1)
    return fail(PAI_ERR_ARG, "pai_mul_dev: bad arguments");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  int rc = ensure_buf(&c->d_mul, &c->mul_bytes, N);
  if (rc) return rc;
  MulParams p{};
  p.ct = d_ct;
  p.exp = d_exp;
  p.m = (long long)N;
  p.d = 1;
  p.cs_i = 1;
  p.xs_i = (long long)x_stride;
  p.x = d_x;
  p.dtype = dtype;
  p.n = (long long)N;
  p.out = d_out;
  p.out_exp = d_exp_out;
  p.status = d_status;
  p.neg = (uint8_t*)c->d_mul;
  if ((rc = launch_mul(c, p, st))) return rc;
  return batch_invert(c, d_out, (const uint8_t*)c->d_mul, (long long)N, st);
}

// E(x) + y over arrays (encrypted_number.py:139-164): k_plain encodes y_i with max_exponent e_i into
// c0_i = 1 + n M_i (r = 1) and E_i, then ONE 2-way k_add aligns E(x_i) to E_i and multiplies.
int pai_add_plain_dev(pai_ctx* c, const uint32_t* d_ct, const int32_t* d_exp, size_t N, int dtype, const void* d_x,
                      size_t x_stride, uint32_t* d_out, int32_t* d_exp_out, int32_t* d_status, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  if (N == 0) return 0;
  if (!d_ct || !d_exp || !d_x || !d_out || !d_exp_out || dtype < 0 || dtype > 2 || x_stride > 1)
    return fail(PAI_ERR_ARG, "pai_add_plain_dev: bad arguments");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t W = c->ct_words, cbytes = align16(2 * N * W * 4);
  int rc = ensure_buf(&c->d_plain, &c->plain_bytes, cbytes + 2 * N * 4);
  if (rc) return rc;
  uint32_t* ops = (uint32_t*)c->d_plain;
  int32_t* oexp = (int32_t*)((char*)c->d_plain + cbytes);
  HIPCHK(hipMemcpyAsync(ops, d_ct, N * W * 4, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(oexp, d_exp, N * 4, hipMemcpyDeviceToDevice, st));
  PlainParams p{};
  p.exp = d_exp;
  p.x = d_x;
  p.dtype = dtype;
  p.xs = (long long)x_stride;
  p.n = (long long)N;
  p.c0 = ops + N * W;
  p.e0 = oexp + N;
  p.status = d_status;
  p.N = c->d_N;
  p.nl = c->d_nl;
  p.ct_words = c->ct_words;
  p.max_bits = c->nb - 3;
  HIPCHK(plain_launch(c->tpi_e, p, (long long)N, c->cus, st));
  return add_dev(c, ops, oexp, 2, (long long)N, d_out, d_exp_out, st);
}

// Segmented k-way add (per-bin sums of IV_FFS, hetero_bin.py:28-36): a reduction tree of
// 16-operand k_add passes whose operands are gathered through a row index (AddParams.gidx), so segments of
// any length share one launch per level. Segment metadata (index, offsets) is host memory.
constexpr int SEG_CHUNK = 16;

int pai_segment_add_dev(pai_ctx* c, const uint32_t* d_ct, const int32_t* d_exp, size_t N, const int64_t* index,
                        const int64_t* seg_off, size_t nseg, uint32_t* d_out, int32_t* d_exp_out, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  if (nseg == 0) return 0;
  if (!d_ct || !d_exp || !seg_off || !d_out || !d_exp_out) return fail(PAI_ERR_ARG, "pai_segment_add_dev: bad arguments");
  if (seg_off[0] != 0) return fail(PAI_ERR_ARG, "pai_segment_add_dev: seg_off[0] must be 0");
  for (size_t s = 0; s < nseg; ++s)
    if (seg_off[s + 1] < seg_off[s]) return fail(PAI_ERR_ARG, "pai_segment_add_dev: offsets must not decrease");
  const long long total = seg_off[nseg];
  if (total > 0 && !index) return fail(PAI_ERR_ARG, "pai_segment_add_dev: index required");
  for (long long t = 0; t < total; ++t)
    if (index[t] < 0 || (size_t)index[t] >= N) return fail(PAI_ERR_ARG, "pai_segment_add_dev: index out of range");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t W = c->ct_words;
  const int C = SEG_CHUNK;
  // members of every segment as source rows; each level maps them to ceil(len / C) partial sums
  std::vector<long long> len(nseg), src(total);
  for (size_t s = 0; s < nseg; ++s) len[s] = seg_off[s + 1] - seg_off[s];
  for (long long t = 0; t < total; ++t) src[t] = index[t];
  long long max_parts = 0;
  for (size_t s = 0; s < nseg; ++s) max_parts += (len[s] + C - 1) / C;
  const size_t o_a = 0, o_b = align16(o_a + (size_t)max_parts * W * 4), o_ea = align16(o_b + (size_t)max_parts * W * 4),
               o_eb = align16(o_ea + (size_t)max_parts * 4), o_g = align16(o_eb + (size_t)max_parts * 4),
               need = align16(o_g + (size_t)std::max<long long>(max_parts, (long long)nseg) * C * 8);
  int rc = ensure_buf(&c->d_seg, &c->seg_bytes, need);
  if (rc) return rc;
  char* b = (char*)c->d_seg;
  uint32_t* part[2] = {(uint32_t*)(b + o_a), (uint32_t*)(b + o_b)};
  int32_t* pexp[2] = {(int32_t*)(b + o_ea), (int32_t*)(b + o_eb)};
  long long* d_g = (long long*)(b + o_g);
  const uint32_t* in = d_ct;
  const int32_t* in_e = d_exp;
  int side = 0;
  std::vector<long long> g;
  for (;;) {
    long long maxlen = 0;
    for (size_t s = 0; s < nseg; ++s) maxlen = std::max(maxlen, len[s]);
    const bool last = maxlen <= C;
    // one gather row of C sources per output (padding -1); the last level has one output per segment
    g.clear();
    std::vector<long long> nlen(nseg), nsrc;
    long long pos = 0;
    for (size_t s = 0; s < nseg; ++s) {
      const long long parts = last ? 1 : (len[s] + C - 1) / C;
      for (long long q = 0; q < parts; ++q) {
        for (int j = 0; j < C; ++j) {
          const long long t = q * C + j;
          g.push_back(t < len[s] ? src[pos + t] : -1);
        }
        nsrc.push_back((long long)nsrc.size());
      }
      pos += len[s];
      nlen[s] = parts;
    }
    const long long outs = (long long)nsrc.size();
    HIPCHK(hipMemcpyAsync(d_g, g.data(), g.size() * 8, hipMemcpyHostToDevice, st));
    uint32_t* o = last ? d_out : part[side];
    int32_t* oe = last ? d_exp_out : pexp[side];
    if ((rc = run_add(c, add_params(in, in_e, C, outs, o, oe, d_g), st))) return rc;
    HIPCHK(hipStreamSynchronize(st));   // the gather rows (host vector) are reused by the next level
    if (last) return 0;
    in = o;
    in_e = oe;
    side ^= 1;
    len.swap(nlen);
    src.swap(nsrc);
  }
}

constexpr int MATMUL_CHUNK = 16;   // operands per k_add pass of the reduction tree

// Bytes of window tables (kernels_mm.hpp k_mm_tab: 16 rows of S limbs per ciphertext, and as many again for the
// inverses once a scalar is negative) that one block of the fused matrix product may hold: 9.25 KiB per ciphertext and
// sign at 2048 bits, so 256 MiB takes 14 k ciphertexts with mixed signs (he_otp_lr's m = 1, K = batch fits many times
// over) and bounds what a context keeps resident. A larger product is processed in blocks of rows i, and a single row
// that is still too long in ranges of k (multiples of MM_KC, at least one chunk); every block writes its own slice of
// the partials, so the reduction tree and the bits do not depend on the blocking.
constexpr size_t MM_TABLE_BYTES = (size_t)256 << 20;

static size_t mm_table_budget() {
  if (const char* e = xcheck_env("FLEXPAI_MM_TABLE_BYTES")) {     // test build: blocking at small shapes
    const unsigned long long v = strtoull(e, nullptr, 10);
    if (v > 0) return (size_t)v;
  }
  return MM_TABLE_BYTES;
}

// Which calls take the fused path (PAI_OPT_MATMUL_FUSED = 1, the default). An instance of k_mm_acc is a chain of about
// 4 nw + 16 nw dependent products where a term of k_mul is one of about 6 nw, so the fused path is faster once the chip
// is full of instances and slower while it is not; and its tables cost 15 products per ciphertext (36 with the inverse)
// that only d columns share. Measured against the parent's term path on an MI355X (tools/mm_ab.py, profiles/mm_ab.json
// and mm_ab_sweep.json; T = K m d terms, G = resident lane groups = 2 blocks x CUs x 256 / TPI): faster by more than
// the spread at d >= 16 with T >= 2 G (1.3x .. 3.5x at 1024, 2048 and 4096 bits), slower at T <= G (0.65x .. 0.93x) and
// at d = 1 whatever T (0.24x .. 0.67x). Calls outside that class keep the term path. The test build sends every call
// through the fused kernels under $FLEXPAI_MM_ALWAYS=1, so that they can be checked at small shapes.
constexpr size_t MM_MIN_D = 16;
constexpr size_t MM_MIN_FILL = 2;

static bool mm_take_fused(const pai_ctx* c, size_t m, size_t K, size_t d) {
  if (!c->mm_fused) return false;
  if (const char* e = xcheck_env("FLEXPAI_MM_ALWAYS"))
    if (atoi(e) != 0) return true;
  const double groups = 2.0 * c->cus * (BLOCK / c->tpi_e);
  return d >= MM_MIN_D && (double)m * (double)K * (double)d >= (double)MM_MIN_FILL * groups;
}

// The fused path of pai_matmul_dev: the ceil(K / MM_KC) chunk partials of every output, [chunk][m d][W] words in
// `part` and [chunk][m d] exponents in `pexp` (the operands of the k_add tree). k_mm_sign's row flags come back to the
// host (one synchronisation of `st`, K bytes: the decision below needs them); only with a negative scalar does the
// call then copy the ciphertexts and invert the flagged rows' (batch_invert: its one synchronisation, and
// PAI_ERR_NOINV exactly where the term path raises it -- a ciphertext without inverse in a row with a negative scalar).
static int matmul_fused(pai_ctx* c, const uint32_t* d_ct, const int32_t* d_exp, size_t m, size_t K, int dtype,
                        const void* d_x, size_t d, uint32_t* part, int32_t* pexp, hipStream_t st) {
  const size_t W = c->ct_words, Np = m * d, nch = (K + MM_KC - 1) / MM_KC;
  const size_t eb = mm_entry_bytes(c->tpi_e);
  if (nch * Np >= (size_t)INT32_MAX) return fail(PAI_ERR_ARG, "pai_matmul_dev: too many partial products");
  const size_t o_flag = align16(K);
  int rc = ensure_buf(&c->d_mmwork, &c->mmwork_bytes, o_flag + align16(m * K));
  if (rc) return rc;
  uint8_t* neg_row = (uint8_t*)c->d_mmwork;
  uint8_t* flags = neg_row + o_flag;
  HIPCHK(hipMemsetAsync(neg_row, 0, K, st));
  MmSignParams sp{};
  sp.x = d_x;
  sp.dtype = dtype;
  sp.K = (long long)K;
  sp.d = (long long)d;
  sp.neg_row = neg_row;
  HIPCHK(mm_sign_launch(sp, c->cus, st));
  c->mm_neg.assign(K, 0);
  HIPCHK(hipMemcpyAsync(c->mm_neg.data(), neg_row, K, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const bool any_neg = std::any_of(c->mm_neg.begin(), c->mm_neg.end(), [](uint8_t v) { return v != 0; });
  uint32_t* inv = nullptr;
  if (any_neg) {
    if ((rc = ensure_buf(&c->d_mminv, &c->mminv_bytes, m * K * W * 4))) return rc;
    inv = (uint32_t*)c->d_mminv;
    c->mm_flags.resize(m * K);
    for (size_t i = 0; i < m; ++i) std::memcpy(c->mm_flags.data() + i * K, c->mm_neg.data(), K);
    HIPCHK(hipMemcpyAsync(flags, c->mm_flags.data(), m * K, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(inv, d_ct, m * K * W * 4, hipMemcpyDeviceToDevice, st));
    if ((rc = batch_invert(c, inv, flags, (long long)(m * K), st))) return rc;
  }
  // blocks: rows first, then ranges of k
  const size_t cap = std::max<size_t>(mm_table_budget() / (eb * (any_neg ? 2 : 1)), 1);   // ciphertexts per block
  size_t mb = m, kb = K;
  if (m * K > cap) {
    if (K <= cap) {
      mb = cap / K;
    } else {
      mb = 1;
      kb = std::max<size_t>(cap / MM_KC, 1) * MM_KC;
    }
  }
  if (mb * kb >= (size_t)INT32_MAX / 2) return fail(PAI_ERR_ARG, "pai_matmul_dev: table block too large");
  if ((rc = ensure_buf(&c->d_mmtab, &c->mmtab_bytes, mb * kb * (any_neg ? 2 : 1) * eb))) return rc;
  for (size_t i0 = 0; i0 < m; i0 += mb) {
    for (size_t k0 = 0; k0 < K; k0 += kb) {
      const size_t mbb = std::min(mb, m - i0), kbb = std::min(kb, K - k0);
      const bool has_neg = any_neg && std::any_of(c->mm_neg.begin() + k0, c->mm_neg.begin() + k0 + kbb,
                                                  [](uint8_t v) { return v != 0; });
      MmTabParams tp{};
      tp.ct = d_ct;
      tp.inv = inv;
      tp.neg_row = neg_row;
      tp.K = (long long)K;
      tp.i0 = (long long)i0;
      tp.k0 = (long long)k0;
      tp.mb = (long long)mbb;
      tp.kb = (long long)kbb;
      tp.has_neg = has_neg ? 1 : 0;
      tp.tab = (uint32_t*)c->d_mmtab;
      tp.N = c->d_N;
      tp.R2 = c->d_R2;
      tp.oneR = c->d_oneR;
      tp.mprime = c->mprime_N;
      tp.ct_words = c->ct_words;
      HIPCHK(mm_tab_launch(c->tpi_e, tp, c->cus, st));
      MmAccParams ap{};
      ap.exp = d_exp;
      ap.x = d_x;
      ap.dtype = dtype;
      ap.K = (long long)K;
      ap.d = (long long)d;
      ap.i0 = (long long)i0;
      ap.k0 = (long long)k0;
      ap.mb = (long long)mbb;
      ap.kb = (long long)kbb;
      ap.has_neg = tp.has_neg;
      ap.tab = tp.tab;
      ap.part = part;
      ap.pexp = pexp;
      ap.Np = (long long)Np;
      ap.N = c->d_N;
      ap.oneR = c->d_oneR;
      ap.mprime = c->mprime_N;
      ap.ct_words = c->ct_words;
      HIPCHK(mm_acc_launch(c->tpi_e, ap, c->cus, st));
    }
  }
  return 0;
}

int pai_matmul_dev(pai_ctx* c, const uint32_t* d_ct, const int32_t* d_exp, size_t m, size_t K, int dtype,
                   const void* d_x, size_t d, uint32_t* d_out, int32_t* d_exp_out, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  if (m == 0 || d == 0) return 0;
  if (K == 0 || !d_ct || !d_exp || !d_x || !d_out || !d_exp_out || dtype < 0 || dtype > 2)
    return fail(PAI_ERR_ARG, "pai_matmul_dev: bad arguments");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t W = c->ct_words, Np = m * d, T = K * Np;
  const int C = MATMUL_CHUNK;
  // fused (kernels_mm.hpp): the term buffer holds the ceil(K / MM_KC) chunk partials instead of the K terms
  const bool fused = mm_take_fused(c, m, K, d);
  c->mm_path = fused ? 2 : 1;
  const size_t rows = fused ? (K + MM_KC - 1) / MM_KC : K;
  const size_t Kp = rows > (size_t)C ? (rows + C - 1) / C * C : rows;   // rows of the term buffer
  const size_t Pr = (Kp + C - 1) / C + C;                              // rows of the partial buffer
  const size_t o_terms = 0, o_texp = align16(o_terms + Kp * Np * W * 4), o_flag = align16(o_texp + Kp * Np * 4),
               o_part = align16(o_flag + (fused ? 0 : T)), o_pexp = align16(o_part + Pr * Np * W * 4), total = align16(o_pexp + Pr * Np * 4);
  int rc = ensure_buf(&c->d_mul, &c->mul_bytes, total);
  if (rc) return rc;
  char* b = (char*)c->d_mul;
  uint32_t* terms = (uint32_t*)(b + o_terms);
  int32_t* texp = (int32_t*)(b + o_texp);
  uint8_t* flag = (uint8_t*)(b + o_flag);
  uint32_t* part = (uint32_t*)(b + o_part);
  int32_t* pexp = (int32_t*)(b + o_pexp);
  if (fused) {
    if ((rc = matmul_fused(c, d_ct, d_exp, m, K, dtype, d_x, d, terms, texp, st))) return rc;
  } else {
    // terms (k, i, j) = c[i][k] (x) x[k][j], k-major: the k_add layout of K operands over m d outputs
    MulParams p{};
    p.ct = d_ct;
    p.exp = d_exp;
    p.m = (long long)m;
    p.d = (long long)d;
    p.cs_i = (long long)K;
    p.cs_k = 1;
    p.xs_k = (long long)d;
    p.xs_j = 1;
    p.x = d_x;
    p.dtype = dtype;
    p.n = (long long)T;
    p.out = terms;
    p.out_exp = texp;
    p.neg = flag;
    if ((rc = launch_mul(c, p, st))) return rc;
    if ((rc = batch_invert(c, terms, flag, (long long)T, st))) return rc;
  }
  // reduction over k: passes of C operands (padding operands: exponent PAD_EXP), then the rest
  uint32_t* cur = terms;
  int32_t* cur_e = texp;
  size_t Kc = rows;
  bool in_terms = true;
  while (Kc > (size_t)C) {
    const size_t Kn = (Kc + C - 1) / C;
    if (Kn * C > Kc) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(cur_e + Kc * Np), PAD_EXP, (Kn * C - Kc) * Np, st));
    uint32_t* nxt = in_terms ? part : terms;
    int32_t* nxt_e = in_terms ? pexp : texp;
    if ((rc = add_dev(c, cur, cur_e, C, (long long)(Kn * Np), nxt, nxt_e, st))) return rc;
    cur = nxt;
    cur_e = nxt_e;
    Kc = Kn;
    in_terms = !in_terms;
  }
  return add_dev(c, cur, cur_e, (int)Kc, (long long)Np, d_out, d_exp_out, st);
}

// ------------------------------------------------------------------ segmented weighted sums (kernels_sd.hpp)
// out_s = sum over t in [seg_off[s], seg_off[s+1]) of ct[index[t]] (x) x[t]. Both paths cut every segment into chunks of
// MM_KC consecutive entries (the last one ragged, none across two segments), write one partial per chunk into a flat
// list and leave the list to the segmented add (identity index, offsets = chunk counts): a partial is the exact residue
// of its chunk at the chunk's largest exponent on either path, so the bits depend neither on the path nor on how the
// chunks are grouped into slices or blocks.
//
//   term path   slices of SD_SLICE_CHUNKS chunks: k_sd_gather copies the slice's ct[index[t]], pai_mul_dev forms the terms
//               (k_mul, one batch inversion) and one pai_segment_add_dev pass sums every chunk
//   fused path  k_sd_sign flags the distinct ciphertexts that meet a negative scalar; blocks of consecutive chunks whose
//               distinct ciphertexts fit the table budget (mm_table_budget, halved once the block holds a flagged one):
//               k_sd_gather compacts them in table-slot order, batch_invert inverts a copy's flagged rows, k_mm_tab
//               builds the tables and k_sd_acc runs the block's chunks
constexpr size_t SD_SLICE_CHUNKS = 8192;   // 131 072 terms: 2 x 64 MiB of term buffer at 2048 bits

// Which calls take the fused path (PAI_OPT_SEGDOT_FUSED = 1, the default). A table costs 15 products (36 with the
// inverse) and pays off over the entries of its block that share it, hence the reuse factor entries / tables in the
// place of pai_matmul's d; a chunk is a chain of about 4 nw + 16 nw dependent products, so a small call takes the
// chain's time whatever its size. Measured on an MI355X against gather + pai_mul_dev + pai_segment_add_dev
// (tools/segdot_ab.py, profiles/segdot_ab.json; 1024 and 2048 bits): faster by more than the spread
// at 65 536 entries and more with reuse >= 16 (1.05x .. 1.4x at 1024 bits, 1.2x .. 1.7x at 2048; 2.1x .. 3.3x from
// 262 144 entries), slower at 16 384 entries and fewer (0.66x .. 0.80x) and at reuse <= 4 whatever the size
// (0.19x .. 0.96x). "Tables" counts what the blocks build: a call whose distinct ciphertexts do not fit one block builds
// a ciphertext's table again in every block that names it (random indices over 16 384 ciphertexts at 2048 bits: 8
// blocks, 0.40x). Calls outside that class keep the term path; 4096-bit keys use the same constants, unmeasured.
constexpr size_t SD_MIN_REUSE = 16;
constexpr size_t SD_MIN_ENTRIES = 65536;

// tables the blocks of segdot_fused build when a block holds at most `limit` distinct ciphertexts
static size_t sd_tables_blocked(const pai_ctx::SdHost& h, size_t limit) {
  std::vector<long long> stamp(h.urows.size(), -1);
  size_t total = 0, nd = 0;
  long long id = 0;
  for (size_t q = 0; q + 1 < h.cstart.size(); ++q) {
    size_t fresh = 0;
    for (long long t = h.cstart[q]; t < h.cstart[q + 1]; ++t)
      if (stamp[h.uid[t]] != id) stamp[h.uid[t]] = id, ++fresh;
    if (nd + fresh > limit && nd > 0) {                             // the chunk opens the next block
      ++id;
      fresh = nd = 0;
      for (long long t = h.cstart[q]; t < h.cstart[q + 1]; ++t)
        if (stamp[h.uid[t]] != id) stamp[h.uid[t]] = id, ++fresh;
    }
    nd += fresh;
    total += fresh;
  }
  return total;
}

static bool sd_take_fused(const pai_ctx* c, size_t nnz) {
  if (!c->sd_fused || nnz == 0) return false;
  if (const char* e = xcheck_env("FLEXPAI_SD_ALWAYS"))
    if (atoi(e) != 0) return true;
  const size_t U = c->sd.urows.size();
  if (nnz < SD_MIN_ENTRIES || nnz < SD_MIN_REUSE * U) return false;
  // signs are not known yet: blocks as if one were present
  const size_t limit = std::max<size_t>(mm_table_budget() / mm_entry_bytes(c->tpi_e) / 2, 1);
  return U <= limit || nnz >= SD_MIN_REUSE * sd_tables_blocked(c->sd, limit);
}

static size_t sd_slice_chunks() {
  if (const char* e = xcheck_env("FLEXPAI_SD_SLICE")) {           // test build: slicing at small shapes
    const unsigned long long v = strtoull(e, nullptr, 10);
    if (v > 0) return (size_t)v;
  }
  return SD_SLICE_CHUNKS;
}

static int sd_gather(pai_ctx* c, const uint32_t* d_ct, const int32_t* d_exp, const long long* d_rows, size_t n,
                     uint32_t* out, int32_t* out_exp, hipStream_t st) {
  SdGatherParams g{};
  g.ct = d_ct;
  g.exp = d_exp;
  g.rows = d_rows;
  g.n = (long long)n;
  g.out = out;
  g.out_exp = out_exp;
  g.ct_words = c->ct_words;
  HIPCHK(sd_gather_launch(g, c->cus, st));
  return 0;
}

// term path: the partials of all chunks, slice by slice (d_index: the index array on the device)
static int segdot_terms(pai_ctx* c, const uint32_t* d_ct, const int32_t* d_exp, const long long* d_index, int dtype,
                        const void* d_x, uint32_t* part, int32_t* pexp, int32_t* d_status, hipStream_t st) {
  auto& h = c->sd;
  const size_t W = c->ct_words, nch = h.cstart.size() - 1, esz = dtype == PAI_F32 ? 4 : 8, slice = sd_slice_chunks();
  const size_t cap = std::min(slice, nch) * MM_KC;                // entries of a slice, at most
  const size_t o_in = 0, o_out = align16(o_in + cap * W * 4), o_ein = align16(o_out + cap * W * 4),
               o_eout = align16(o_ein + cap * 4), need = align16(o_eout + cap * 4);
  int rc = ensure_buf(&c->d_sdbuf, &c->sdbuf_bytes, need);
  if (rc) return rc;
  char* b = (char*)c->d_sdbuf;
  uint32_t *tin = (uint32_t*)(b + o_in), *tout = (uint32_t*)(b + o_out);
  int32_t *ein = (int32_t*)(b + o_ein), *eout = (int32_t*)(b + o_eout);
  std::vector<long long> off;
  for (size_t qa = 0; qa < nch; qa += slice) {
    const size_t qb = std::min(nch, qa + slice);
    const long long ta = h.cstart[qa], n = h.cstart[qb] - ta;
    if ((rc = sd_gather(c, d_ct, d_exp, d_index + ta, (size_t)n, tin, ein, st))) return rc;
    if ((rc = pai_mul_dev(c, tin, ein, (size_t)n, dtype, (const char*)d_x + (size_t)ta * esz, 1, tout, eout,
                          d_status ? d_status + ta : nullptr, st)))
      return rc;
    off.resize(qb - qa + 1);
    for (size_t q = qa; q <= qb; ++q) off[q - qa] = h.cstart[q] - ta;
    // (synchronises `st` before it returns: `off` may be rewritten)
    if ((rc = pai_segment_add_dev(c, tout, eout, (size_t)n, (const int64_t*)h.iota.data(), (const int64_t*)off.data(), qb - qa,
                                  part + qa * W, pexp + qa, st)))
      return rc;
  }
  return 0;
}

// fused path: the partials of all chunks, block by block. d_index, d_cstart: the device sides of index and of the chunk
// starts; d_uid [nnz]: room for the entries' distinct ids, which the table slots overwrite once the signs are known.
static int segdot_fused(pai_ctx* c, const uint32_t* d_ct, const int32_t* d_exp, const long long* d_index,
                        const long long* d_cstart, int32_t* d_uid, size_t nnz, int dtype, const void* d_x, uint32_t* part,
                        int32_t* pexp, int32_t* d_status, hipStream_t st) {
  auto& h = c->sd;
  const size_t W = c->ct_words, nch = h.cstart.size() - 1, U = h.urows.size(), eb = mm_entry_bytes(c->tpi_e);
  // signs (and pai_mul's statuses) of the entries -> flags of the distinct ciphertexts
  // sdbuf: [neg | block rows | block flags | the block's ciphertexts]; the rows of all blocks together are at most nnz
  const size_t o_neg = 0, o_rows = align16(o_neg + U), o_flags = align16(o_rows + nnz * 8), o_ct = align16(o_flags + nnz);
  int rc = ensure_buf(&c->d_sdbuf, &c->sdbuf_bytes, o_ct);
  if (rc) return rc;
  uint8_t* d_neg = (uint8_t*)c->d_sdbuf + o_neg;
  HIPCHK(hipMemsetAsync(d_neg, 0, U, st));
  HIPCHK(hipMemcpyAsync(d_uid, h.uid.data(), nnz * 4, hipMemcpyHostToDevice, st));
  SdSignParams sp{};
  sp.x = d_x;
  sp.dtype = dtype;
  sp.nnz = (long long)nnz;
  sp.uid = d_uid;
  sp.neg = d_neg;
  sp.status = d_status;
  HIPCHK(sd_sign_launch(sp, c->cus, st));
  h.neg.assign(U, 0);
  HIPCHK(hipMemcpyAsync(h.neg.data(), d_neg, U, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));

  // blocks of consecutive chunks; every block numbers its distinct ciphertexts in order of first use
  struct Block {
    size_t q0, q1, roff, nd;
    bool has_neg;
  };
  std::vector<Block> blocks;
  const size_t cap = std::max<size_t>(mm_table_budget() / eb, 1);
  std::vector<long long> stamp(U, -1);
  std::vector<int32_t> slot_of(U, 0);
  h.rows.clear();
  h.tslot.resize(nnz);
  for (size_t q = 0; q < nch;) {
    Block b{q, q, h.rows.size(), 0, false};
    const long long id = (long long)blocks.size();
    for (; q < nch; ++q) {
      const size_t before = h.rows.size();
      bool hn = b.has_neg;
      for (long long t = h.cstart[q]; t < h.cstart[q + 1]; ++t) {
        const int32_t u = h.uid[t];
        if (stamp[u] != id) {
          stamp[u] = id;
          slot_of[u] = (int32_t)(h.rows.size() - b.roff);
          h.rows.push_back(u);
          hn = hn || h.neg[u] != 0;
        }
      }
      const size_t limit = std::max<size_t>(hn ? cap / 2 : cap, 1);
      if (h.rows.size() - b.roff > limit && q > b.q0) {             // the chunk opens the next block
        for (size_t r = before; r < h.rows.size(); ++r) stamp[h.rows[r]] = -1;
        h.rows.resize(before);
        break;
      }
      b.has_neg = hn;
      for (long long t = h.cstart[q]; t < h.cstart[q + 1]; ++t) h.tslot[t] = slot_of[h.uid[t]];
    }
    b.q1 = q;
    b.nd = h.rows.size() - b.roff;
    blocks.push_back(b);
  }
  size_t max_nd = 1, max_tab = 1;
  for (const Block& b : blocks) {
    max_nd = std::max(max_nd, b.nd);
    max_tab = std::max(max_tab, b.nd * (b.has_neg ? 2 : 1));
  }
  if (max_tab >= (size_t)INT32_MAX / 2) return fail(PAI_ERR_ARG, "pai_segment_dot_dev: table block too large");
  h.flags.resize(h.rows.size());
  for (size_t r = 0; r < h.rows.size(); ++r) {
    h.flags[r] = h.neg[h.rows[r]];
    h.rows[r] = h.urows[h.rows[r]];                                 // distinct id -> row of ct
  }
  if ((rc = ensure_buf(&c->d_sdbuf, &c->sdbuf_bytes, o_ct + max_nd * W * 4))) return rc;
  char* sb = (char*)c->d_sdbuf;
  long long* d_rows = (long long*)(sb + o_rows);
  uint8_t* d_flags = (uint8_t*)(sb + o_flags);
  uint32_t* cbuf = (uint32_t*)(sb + o_ct);
  if ((rc = ensure_buf(&c->d_mmtab, &c->mmtab_bytes, max_tab * eb))) return rc;
  HIPCHK(hipMemcpyAsync(d_uid, h.tslot.data(), nnz * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_rows, h.rows.data(), h.rows.size() * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_flags, h.flags.data(), h.flags.size(), hipMemcpyHostToDevice, st));
  for (const Block& b : blocks) {
    if ((rc = sd_gather(c, d_ct, nullptr, d_rows + b.roff, b.nd, cbuf, nullptr, st))) return rc;
    uint32_t* inv = nullptr;
    if (b.has_neg) {
      if ((rc = ensure_buf(&c->d_mminv, &c->mminv_bytes, max_nd * W * 4))) return rc;
      inv = (uint32_t*)c->d_mminv;
      HIPCHK(hipMemcpyAsync(inv, cbuf, b.nd * W * 4, hipMemcpyDeviceToDevice, st));
      if ((rc = batch_invert(c, inv, d_flags + b.roff, (long long)b.nd, st))) return rc;
    }
    MmTabParams tp{};
    tp.ct = cbuf;
    tp.inv = inv;
    tp.neg_row = d_flags + b.roff;
    tp.K = (long long)b.nd;
    tp.mb = 1;
    tp.kb = (long long)b.nd;
    tp.has_neg = b.has_neg ? 1 : 0;
    tp.tab = (uint32_t*)c->d_mmtab;
    tp.N = c->d_N;
    tp.R2 = c->d_R2;
    tp.oneR = c->d_oneR;
    tp.mprime = c->mprime_N;
    tp.ct_words = c->ct_words;
    HIPCHK(mm_tab_launch(c->tpi_e, tp, c->cus, st));
    SdAccParams ap{};
    ap.exp = d_exp;
    ap.x = d_x;
    ap.dtype = dtype;
    ap.index = d_index;
    ap.tslot = d_uid;
    ap.cstart = d_cstart;
    ap.q0 = (int)b.q0;
    ap.q1 = (int)b.q1;
    ap.ne = (int)b.nd;
    ap.tab = tp.tab;
    ap.part = part;
    ap.pexp = pexp;
    ap.N = c->d_N;
    ap.oneR = c->d_oneR;
    ap.mprime = c->mprime_N;
    ap.ct_words = c->ct_words;
    HIPCHK(sd_acc_launch(c->tpi_e, ap, c->cus, st));
  }
  return 0;
}

int pai_segment_dot_dev(pai_ctx* c, const uint32_t* d_ct, const int32_t* d_exp, size_t N, const int64_t* index,
                        const int64_t* seg_off, size_t nseg, int dtype, const void* d_x, uint32_t* d_out,
                        int32_t* d_exp_out, int32_t* d_status, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  if (nseg == 0) return 0;
  if (!seg_off || !d_out || !d_exp_out || dtype < 0 || dtype > 2) return fail(PAI_ERR_ARG, "pai_segment_dot_dev: bad arguments");
  if (seg_off[0] != 0) return fail(PAI_ERR_ARG, "pai_segment_dot_dev: seg_off[0] must be 0");
  for (size_t s = 0; s < nseg; ++s)
    if (seg_off[s + 1] < seg_off[s]) return fail(PAI_ERR_ARG, "pai_segment_dot_dev: offsets must not decrease");
  const size_t nnz = (size_t)seg_off[nseg];
  if (nnz > 0 && (!d_ct || !d_exp || !index || !d_x)) return fail(PAI_ERR_ARG, "pai_segment_dot_dev: bad arguments");
  for (size_t t = 0; t < nnz; ++t)
    if (index[t] < 0 || (size_t)index[t] >= N) return fail(PAI_ERR_ARG, "pai_segment_dot_dev: index out of range");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t W = c->ct_words;
  auto& h = c->sd;
  // chunks: ceil(len / MM_KC) per segment, consecutive
  h.cstart.clear();
  h.segch.assign(1, 0);
  for (size_t s = 0; s < nseg; ++s) {
    for (long long t = seg_off[s]; t < seg_off[s + 1]; t += MM_KC) h.cstart.push_back(t);
    h.segch.push_back((long long)h.cstart.size());
  }
  h.cstart.push_back((long long)nnz);
  const size_t nch = h.cstart.size() - 1;
  if (nch >= (size_t)INT32_MAX) return fail(PAI_ERR_ARG, "pai_segment_dot_dev: too many partial products");
  h.iota.resize(std::max(nch, std::min(nch, sd_slice_chunks()) * MM_KC));
  for (size_t i = 0; i < h.iota.size(); ++i) h.iota[i] = (long long)i;
  // the distinct ciphertexts of the call (urows) and every entry's place among them (uid): in order of first use
  // through a map over the N rows, or ascending through a sort where N dwarfs the entries
  h.uid.resize(nnz);
  if (N / 8 <= nnz + 4096) {
    h.idmap.assign(N, -1);
    h.urows.clear();
    for (size_t t = 0; t < nnz; ++t) {
      int32_t& u = h.idmap[(size_t)index[t]];
      if (u < 0) {
        if (h.urows.size() >= (size_t)INT32_MAX - 1) return fail(PAI_ERR_ARG, "pai_segment_dot_dev: too many ciphertexts");
        u = (int32_t)h.urows.size();
        h.urows.push_back((long long)index[t]);
      }
      h.uid[t] = u;
    }
  } else {
    h.urows.assign(index, index + nnz);
    std::sort(h.urows.begin(), h.urows.end());
    h.urows.erase(std::unique(h.urows.begin(), h.urows.end()), h.urows.end());
    if (h.urows.size() >= (size_t)INT32_MAX) return fail(PAI_ERR_ARG, "pai_segment_dot_dev: too many ciphertexts");
    for (size_t t = 0; t < nnz; ++t)
      h.uid[t] = (int32_t)(std::lower_bound(h.urows.begin(), h.urows.end(), (long long)index[t]) - h.urows.begin());
  }
  const bool fused = sd_take_fused(c, nnz);
  c->sd_path = fused ? 2 : 1;
  const size_t o_pexp = align16(std::max<size_t>(nch, 1) * W * 4);
  int rc = ensure_buf(&c->d_sdpart, &c->sdpart_bytes, o_pexp + align16(std::max<size_t>(nch, 1) * 4));
  if (rc) return rc;
  uint32_t* part = (uint32_t*)c->d_sdpart;
  int32_t* pexp = (int32_t*)((char*)c->d_sdpart + o_pexp);
  if (nnz > 0) {
    const size_t o_cs = align16(nnz * 8), o_uid = align16(o_cs + (nch + 1) * 8);
    if ((rc = ensure_buf(&c->d_sdmeta, &c->sdmeta_bytes, o_uid + align16(nnz * 4)))) return rc;
    long long* d_index = (long long*)c->d_sdmeta;
    long long* d_cstart = (long long*)((char*)c->d_sdmeta + o_cs);
    int32_t* d_uid = (int32_t*)((char*)c->d_sdmeta + o_uid);
    static_assert(sizeof(long long) == sizeof(int64_t), "index upload");
    HIPCHK(hipMemcpyAsync(d_index, index, nnz * 8, hipMemcpyHostToDevice, st));
    if (fused) {
      HIPCHK(hipMemcpyAsync(d_cstart, h.cstart.data(), (nch + 1) * 8, hipMemcpyHostToDevice, st));
      rc = segdot_fused(c, d_ct, d_exp, d_index, d_cstart, d_uid, nnz, dtype, d_x, part, pexp, d_status, st);
    } else {
      rc = segdot_terms(c, d_ct, d_exp, d_index, dtype, d_x, part, pexp, d_status, st);
    }
    if (rc) {
      (void)hipStreamSynchronize(st);   // the caller's index array may go once the call has returned
      return rc;
    }
  }
  // the partials of segment s are rows segch[s] .. segch[s + 1]; an empty segment has none (ciphertext 1, INT32_MIN)
  return pai_segment_add_dev(c, part, pexp, nch, (const int64_t*)h.iota.data(), (const int64_t*)h.segch.data(), nseg, d_out,
                             d_exp_out, stream);
}

int pai_mul(pai_ctx* c, const uint32_t* ct, const int32_t* exp, size_t N, int dtype, const void* x, size_t x_stride,
            uint32_t* ct_out, int32_t* exp_out, int32_t* status_out) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (N == 0) return 0;
  if (!ct || !exp || !x || !ct_out || !exp_out || x_stride > 1) return fail(PAI_ERR_ARG, "pai_mul: bad arguments");
  HIPCHK(hipSetDevice(c->device));
  const size_t W = c->ct_words, esz = dtype == PAI_F32 ? 4 : 8, nx = x_stride ? N : 1;
  DevScope ds;
  uint32_t* dct = ds.alloc<uint32_t>(N * W);
  int32_t* dexp = ds.alloc<int32_t>(N);
  void* dx = ds.alloc<uint8_t>(nx * esz);
  uint32_t* dout = ds.alloc<uint32_t>(N * W);
  int32_t* dexo = ds.alloc<int32_t>(N);
  int32_t* dst = ds.alloc<int32_t>(N);
  if (!dct || !dexp || !dx || !dout || !dexo || !dst) return fail(PAI_ERR_HIP, "pai_mul: device allocation failed");
  HIPCHK(hipMemcpy(dct, ct, N * W * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dexp, exp, N * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dx, x, nx * esz, hipMemcpyHostToDevice));
  int rc = pai_mul_dev(c, dct, dexp, N, dtype, dx, x_stride, dout, dexo, dst, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(ct_out, dout, N * W * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(exp_out, dexo, N * 4, hipMemcpyDeviceToHost));
  if (status_out) HIPCHK(hipMemcpy(status_out, dst, N * 4, hipMemcpyDeviceToHost));
  return 0;
}

int pai_add_plain(pai_ctx* c, const uint32_t* ct, const int32_t* exp, size_t N, int dtype, const void* x,
                  size_t x_stride, uint32_t* ct_out, int32_t* exp_out, int32_t* status_out) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (N == 0) return 0;
  if (!ct || !exp || !x || !ct_out || !exp_out || x_stride > 1) return fail(PAI_ERR_ARG, "pai_add_plain: bad arguments");
  HIPCHK(hipSetDevice(c->device));
  const size_t W = c->ct_words, esz = dtype == PAI_F32 ? 4 : 8, nx = x_stride ? N : 1;
  DevScope ds;
  uint32_t* dct = ds.alloc<uint32_t>(N * W);
  int32_t* dexp = ds.alloc<int32_t>(N);
  void* dx = ds.alloc<uint8_t>(nx * esz);
  uint32_t* dout = ds.alloc<uint32_t>(N * W);
  int32_t* dexo = ds.alloc<int32_t>(N);
  int32_t* dst = ds.alloc<int32_t>(N);
  if (!dct || !dexp || !dx || !dout || !dexo || !dst) return fail(PAI_ERR_HIP, "pai_add_plain: device allocation failed");
  HIPCHK(hipMemcpy(dct, ct, N * W * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dexp, exp, N * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dx, x, nx * esz, hipMemcpyHostToDevice));
  int rc = pai_add_plain_dev(c, dct, dexp, N, dtype, dx, x_stride, dout, dexo, dst, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(ct_out, dout, N * W * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(exp_out, dexo, N * 4, hipMemcpyDeviceToHost));
  if (status_out) HIPCHK(hipMemcpy(status_out, dst, N * 4, hipMemcpyDeviceToHost));
  return 0;
}

int pai_segment_add(pai_ctx* c, const uint32_t* ct, const int32_t* exp, size_t N, const int64_t* index,
                    const int64_t* seg_off, size_t nseg, uint32_t* ct_out, int32_t* exp_out) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (nseg == 0) return 0;
  if ((N && (!ct || !exp)) || !seg_off || !ct_out || !exp_out) return fail(PAI_ERR_ARG, "pai_segment_add: bad arguments");
  HIPCHK(hipSetDevice(c->device));
  const size_t W = c->ct_words;
  DevScope ds;
  uint32_t* dct = ds.alloc<uint32_t>(N * W);
  int32_t* dexp = ds.alloc<int32_t>(N);
  uint32_t* dout = ds.alloc<uint32_t>(nseg * W);
  int32_t* dexo = ds.alloc<int32_t>(nseg);
  if (!dct || !dexp || !dout || !dexo) return fail(PAI_ERR_HIP, "pai_segment_add: device allocation failed");
  if (N) {
    HIPCHK(hipMemcpy(dct, ct, N * W * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dexp, exp, N * 4, hipMemcpyHostToDevice));
  }
  int rc = pai_segment_add_dev(c, dct, dexp, N, index, seg_off, nseg, dout, dexo, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(ct_out, dout, nseg * W * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(exp_out, dexo, nseg * 4, hipMemcpyDeviceToHost));
  return 0;
}

// ------------------------------------------------------------------ histograms (kernels_hist.hpp)
// Cell sums of one ciphertext vector over an [N][F] matrix of bin ids and an optional node id per sample. The counts
// of all cells come back to the host once (k_hist_count; the closing segmented add needs host offsets anyway); every
// cell is cut into runs of HIST_RUN members. The features are then processed in blocks whose member lists fit the
// scratch budget: k_hist_scatter places the sample ids and one k_hist_acc launch reads the lists and writes a canonical
// partial per run at the run's largest exponent (the test build's other variant: k_hist_rows turns the runs into gather
// rows, which then count towards the budget, and k_add sums them). A partial is the exact
// residue of its run, so the bits depend neither on the order inside a list nor on runs or blocks. The runs of a cell
// are consecutive rows of its block; the closing pai_segment_add_dev names them through an index of one entry per RUN
// (the identity when the call is one block).
//
// HIST_MAX_CELLS: counts, member offsets and cursors take 16 bytes per cell on the device and 28 on the host, and the
// outputs W words: 2^24 cells are 8 GiB of output at 2048 bits, beyond which no caller's buffer goes.
constexpr size_t HIST_MAX_CELLS = (size_t)1 << 24;
constexpr size_t HIST_HOST_CHUNK = 65536;          // samples per chunk of the host-buffer variant
constexpr size_t HIST_HOST_PART_BYTES = (size_t)1 << 30;   // bound on the chunks' cell sums of the host-buffer variant

static size_t hist_budget(const pai_ctx* c) {
  if (const char* e = xcheck_env("FLEXPAI_HIST_SCRATCH_BYTES")) {   // test build: feature blocks at small shapes
    const unsigned long long v = strtoull(e, nullptr, 10);
    if (v > 0) return (size_t)v;
  }
  return c->hist_scratch;
}

// The variant that sums the runs (test build: $FLEXPAI_HIST_ACC = 0 k_hist_rows + k_add over runs of HIST_RUN,
// 1 k_hist_acc) and the run length of k_hist_acc ($FLEXPAI_HIST_RUN); same bits whichever is taken. The defaults are
// the fastest of tools/hist_ab.py on N = 262 144, F = 16, B = 32 (profiles/hist_ab.json): k_hist_acc
// over runs of 64 takes 3.8 ms at 1024 bits and 10.1 ms at 2048 where k_add over gather rows takes 4.2 and 10.3, runs of
// 128 take 4.6 and 11.1 and runs of 256 take 5.5 and 14.1 (4 M members in runs of 256 are 16 384 lane groups, fewer than
// the chip holds).
constexpr bool HIST_ACC_DEFAULT = true;
static bool hist_use_acc() {
  if (const char* e = xcheck_env("FLEXPAI_HIST_ACC")) return atoi(e) != 0;
  return HIST_ACC_DEFAULT;
}
static size_t hist_run_len(bool acc) {
  if (acc)
    if (const char* e = xcheck_env("FLEXPAI_HIST_RUN")) {
      const unsigned long long v = strtoull(e, nullptr, 10);
      if (v >= 1 && v <= 65536) return (size_t)v;
    }
  return HIST_RUN;
}

static int hist_check(const void* ct, const void* exp, size_t N, int bin_dtype, const void* bins, size_t F, size_t bin_stride,
                      const int32_t* node, size_t nodes, size_t B, const void* ct_out, const void* exp_out, const char* who) {
  const std::string w(who);
  if ((N && (!ct || !exp || !bins)) || !ct_out || !exp_out) return fail(PAI_ERR_ARG, w + ": null pointer");
  if (bin_dtype != PAI_BIN_U8 && bin_dtype != PAI_BIN_U16) return fail(PAI_ERR_ARG, w + ": bin_dtype must be PAI_BIN_U8 or PAI_BIN_U16");
  if (F == 0 || bin_stride < F) return fail(PAI_ERR_ARG, w + ": bin_stride must be at least F >= 1");
  if (B == 0 || B > (bin_dtype == PAI_BIN_U8 ? (size_t)256 : (size_t)65536)) return fail(PAI_ERR_ARG, w + ": B out of range for the bin type");
  if (nodes == 0 || (!node && nodes != 1)) return fail(PAI_ERR_ARG, w + ": nodes must be >= 1, and 1 without node ids");
  if (nodes > HIST_MAX_CELLS || F > HIST_MAX_CELLS || nodes * F > HIST_MAX_CELLS || nodes * F * B > HIST_MAX_CELLS)
    return fail(PAI_ERR_ARG, w + ": more than 2^24 cells");
  if (N >= ((size_t)1 << 31) || N * F >= ((size_t)1 << 31)) return fail(PAI_ERR_ARG, w + ": N F must be below 2^31");
  if (N && (N - 1) > (SIZE_MAX / 2 - F) / bin_stride) return fail(PAI_ERR_ARG, w + ": bin matrix too large");
  return 0;
}

// The cell sums of nodes x F x B member lists over N ciphertexts. `count(d_cnt)` launches the pass that adds the members
// per cell to the zeroed counters, `counted()` runs on the host once `st` has been synchronised for them, and
// `scatter(f0, f1, d_cnt, d_off, d_cur, d_mem)` fills the member lists of one feature block. A cell holds at most N
// members.
template <typename Count, typename Counted, typename Scatter>
static int hist_lists_dev(pai_ctx* c, const std::string& who, const uint32_t* d_ct, const int32_t* d_exp, size_t N, size_t F,
                          size_t nodes, size_t B, Count&& count, Counted&& counted, Scatter&& scatter, uint32_t* d_out,
                          int32_t* d_exp_out, int64_t* d_count_out, hipStream_t st) {
  int rc = 0;
  const bool acc = hist_use_acc();
  const size_t W = c->ct_words, cells = nodes * F * B, R = hist_run_len(acc), row_bytes = acc ? 0 : R * 8;
  auto& h = c->hist;
  // counts of all cells
  const size_t o_off = d_count_out ? 0 : align16(cells * 8), o_cur = align16(o_off + cells * 4), o_runs = align16(o_cur + cells * 4);
  if ((rc = ensure_buf(&c->d_histmeta, &c->histmeta_bytes, o_runs))) return rc;
  unsigned long long* d_cnt = d_count_out ? (unsigned long long*)d_count_out : (unsigned long long*)c->d_histmeta;
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "count_out");
  HIPCHK(hipMemsetAsync(d_cnt, 0, cells * 8, st));
  h.cnt.assign(cells, 0);
  if (N) {
    if ((rc = count(d_cnt))) return rc;
    HIPCHK(hipMemcpyAsync(h.cnt.data(), d_cnt, cells * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if ((rc = counted())) return rc;
  }
  // feature blocks: members (4 bytes each) and k_add's gather rows (8 R bytes per run) within the budget, one feature
  // at least
  struct Block {
    size_t f0, f1, entries, runs, row0;
  };
  std::vector<Block> blocks;
  const size_t budget = hist_budget(c);
  size_t total_runs = 0;
  {
    Block b{0, 0, 0, 0, 0};
    for (size_t f = 0; f < F; ++f) {
      size_t ent = 0, runs = 0;
      for (size_t v = 0; v < nodes; ++v)
        for (size_t q = 0; q < B; ++q) {
          const long long n = h.cnt[(v * F + f) * B + q];
          if (n < 0 || (size_t)n > N) return fail(PAI_ERR_HIP, who + ": cell count out of range");
          ent += (size_t)n;
          runs += ((size_t)n + R - 1) / R;
        }
      if (b.f1 > b.f0 && (b.entries + ent) * 4 + (b.runs + runs) * row_bytes > budget) {
        blocks.push_back(b);
        total_runs += b.runs;
        b = Block{f, f, 0, 0, total_runs};
      }
      b.f1 = f + 1;
      b.entries += ent;
      b.runs += runs;
    }
    blocks.push_back(b);
    total_runs += b.runs;
  }
  if (total_runs >= (size_t)INT32_MAX) return fail(PAI_ERR_ARG, who + ": too many runs");
  // member offsets (relative to the block's list) and runs in block order (v, f, b); the cells' partial rows
  h.cell_off.assign(cells, 0);
  h.runs.clear();
  h.runs.reserve(total_runs);
  std::vector<long long>& row0 = h.index;   // first: the first partial row of every cell
  row0.assign(cells, 0);
  size_t max_ent = 1, max_runs = 1;
  for (const Block& b : blocks) {
    size_t off = 0;
    for (size_t v = 0; v < nodes; ++v)
      for (size_t f = b.f0; f < b.f1; ++f)
        for (size_t q = 0; q < B; ++q) {
          const size_t cell = (v * F + f) * B + q, n = (size_t)h.cnt[cell];
          h.cell_off[cell] = (int32_t)off;
          row0[cell] = (long long)h.runs.size();
          for (size_t t = 0; t < n; t += R) h.runs.push_back(make_int2((int)(off + t), (int)std::min(R, n - t)));
          off += n;
        }
    max_ent = std::max(max_ent, b.entries);
    max_runs = std::max(max_runs, b.runs);
  }
  h.segoff.assign(cells + 1, 0);
  for (size_t cell = 0; cell < cells; ++cell) h.segoff[cell + 1] = h.segoff[cell] + (long long)(((size_t)h.cnt[cell] + R - 1) / R);
  {
    std::vector<long long> idx(total_runs);
    for (size_t cell = 0; cell < cells; ++cell)
      for (long long q = h.segoff[cell]; q < h.segoff[cell + 1]; ++q) idx[q] = row0[cell] + (q - h.segoff[cell]);
    h.index.swap(idx);
  }
  if (total_runs) {
    if ((rc = ensure_buf(&c->d_histmeta, &c->histmeta_bytes, o_runs + align16(total_runs * 8)))) return rc;
    // (a grown buffer lost the counts it may have held: they are on the host)
    if (!d_count_out) {
      d_cnt = (unsigned long long*)c->d_histmeta;
      HIPCHK(hipMemcpyAsync(d_cnt, h.cnt.data(), cells * 8, hipMemcpyHostToDevice, st));
    }
  }
  char* mb = (char*)c->d_histmeta;
  int32_t* d_off = (int32_t*)(mb + o_off);
  unsigned* d_cur = (unsigned*)(mb + o_cur);
  int2* d_runs = (int2*)(mb + o_runs);
  const size_t o_g = align16(max_ent * 4);
  if ((rc = ensure_buf(&c->d_histwork, &c->histwork_bytes, o_g + max_runs * row_bytes))) return rc;
  int32_t* d_mem = (int32_t*)c->d_histwork;
  long long* d_g = (long long*)((char*)c->d_histwork + o_g);
  const size_t o_pexp = align16(std::max<size_t>(total_runs, 1) * W * 4);
  if ((rc = ensure_buf(&c->d_histpart, &c->histpart_bytes, o_pexp + align16(std::max<size_t>(total_runs, 1) * 4)))) return rc;
  uint32_t* part = (uint32_t*)c->d_histpart;
  int32_t* pexp = (int32_t*)((char*)c->d_histpart + o_pexp);
  if (total_runs) {
    HIPCHK(hipMemcpyAsync(d_off, h.cell_off.data(), cells * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_cur, 0, cells * 4, st));
    HIPCHK(hipMemcpyAsync(d_runs, h.runs.data(), total_runs * 8, hipMemcpyHostToDevice, st));
    for (const Block& b : blocks) {
      if (!b.runs) continue;
      HIPCHK(hipMemsetAsync(d_mem, 0, b.entries * 4, st));
      HIPCHK(scatter(b.f0, b.f1, d_cnt, d_off, d_cur, d_mem));
      if (acc) {
        HistAccParams ap{};
        ap.cts = d_ct;
        ap.exps = d_exp;
        ap.members = d_mem;
        ap.runs = d_runs + b.row0;
        ap.nruns = (long long)b.runs;
        ap.out = part + b.row0 * W;
        ap.out_exp = pexp + b.row0;
        ap.N = c->d_N;
        ap.RS = c->d_RS;
        ap.mprime = c->mprime_N;
        ap.ct_words = c->ct_words;
        HIPCHK(hist_acc_launch(c->tpi_e, ap, c->cus, st));
        continue;
      }
      HistRowsParams rp{};
      rp.members = d_mem;
      rp.runs = d_runs + b.row0;
      rp.nruns = (long long)b.runs;
      rp.gidx = d_g;
      HIPCHK(hist_rows_launch(rp, c->cus, st));
      if ((rc = run_add(c, add_params(d_ct, d_exp, HIST_RUN, (long long)b.runs, part + b.row0 * W, pexp + b.row0, d_g), st))) {
        (void)hipStreamSynchronize(st);
        return rc;
      }
    }
  }
  // the partials of cell s are rows index[segoff[s] .. segoff[s + 1]); an empty cell has none (ciphertext 1, INT32_MIN)
  return pai_segment_add_dev(c, part, pexp, total_runs, (const int64_t*)h.index.data(), (const int64_t*)h.segoff.data(), cells, d_out,
                             d_exp_out, (void*)st);
}

int pai_histogram_dev(pai_ctx* c, const uint32_t* d_ct, const int32_t* d_exp, size_t N, int bin_dtype, const void* d_bins,
                      size_t F, size_t bin_stride, const int32_t* d_node, size_t nodes, size_t B, uint32_t* d_out,
                      int32_t* d_exp_out, int64_t* d_count_out, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  int rc = hist_check(d_ct, d_exp, N, bin_dtype, d_bins, F, bin_stride, d_node, nodes, B, d_out, d_exp_out, "pai_histogram_dev");
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  HistParams hp{};
  hp.bins = d_bins;
  hp.bin_u16 = bin_dtype == PAI_BIN_U16 ? 1 : 0;
  hp.stride = (long long)bin_stride;
  hp.node = d_node;
  hp.nodes = (int)nodes;
  hp.B = (int)B;
  hp.N = (long long)N;
  hp.F = (long long)F;
  auto count = [&](unsigned long long* d_cnt) -> int {
    hp.count = d_cnt;
    hp.f0 = 0;
    hp.f1 = (long long)F;
    HIPCHK(hist_count_launch(hp, c->cus, st));
    return 0;
  };
  auto scatter = [&](size_t f0, size_t f1, unsigned long long* d_cnt, const int32_t* d_off, unsigned* d_cur, int32_t* d_mem) {
    hp.count = d_cnt;
    hp.cell_off = d_off;
    hp.cursor = d_cur;
    hp.members = d_mem;
    hp.f0 = (long long)f0;
    hp.f1 = (long long)f1;
    return hist_scatter_launch(hp, c->cus, st);
  };
  return hist_lists_dev(c, "pai_histogram_dev", d_ct, d_exp, N, F, nodes, B, count, [] { return 0; }, scatter, d_out, d_exp_out,
                        d_count_out, st);
}

int pai_histogram(pai_ctx* c, const uint32_t* ct, const int32_t* exp, size_t N, int bin_dtype, const void* bins, size_t F,
                  size_t bin_stride, const int32_t* node, size_t nodes, size_t B, uint32_t* ct_out, int32_t* exp_out,
                  int64_t* count_out) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  int rc = hist_check(ct, exp, N, bin_dtype, bins, F, bin_stride, node, nodes, B, ct_out, exp_out, "pai_histogram");
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  const size_t W = c->ct_words, cells = nodes * F * B, bsz = bin_dtype == PAI_BIN_U16 ? 2 : 1;
  // chunks of samples; their cell sums [chunk][cells] are the operands of one k-way add (an empty cell: PAD_EXP)
  size_t chunk = HIST_HOST_CHUNK;
  if (const char* e = xcheck_env("FLEXPAI_HIST_CHUNK")) {           // test build: chunks at small shapes
    const unsigned long long v = strtoull(e, nullptr, 10);
    if (v > 0) chunk = (size_t)v;
  }
  const size_t kmax = std::max<size_t>(HIST_HOST_PART_BYTES / (cells * W * 4), 1);
  if ((N + chunk - 1) / chunk > kmax) chunk = (N + kmax - 1) / kmax;
  const size_t k = std::max<size_t>((N + chunk - 1) / chunk, 1), nc = std::min(chunk, std::max<size_t>(N, 1));
  DevScope ds;
  uint32_t* dct = ds.alloc<uint32_t>(nc * W);
  int32_t* dexp = ds.alloc<int32_t>(nc);
  uint8_t* dbins = ds.alloc<uint8_t>(nc * bin_stride * bsz);
  int32_t* dnode = node ? ds.alloc<int32_t>(nc) : nullptr;
  uint32_t* dpart = ds.alloc<uint32_t>(k * cells * W);
  int32_t* dpexp = ds.alloc<int32_t>(k * cells);
  int64_t* dcnt = ds.alloc<int64_t>(cells);
  uint32_t* dout = k > 1 ? ds.alloc<uint32_t>(cells * W) : dpart;
  int32_t* dexo = k > 1 ? ds.alloc<int32_t>(cells) : dpexp;
  if (!dct || !dexp || !dbins || (node && !dnode) || !dpart || !dpexp || !dcnt || !dout || !dexo)
    return fail(PAI_ERR_HIP, "pai_histogram: device allocation failed");
  std::vector<int64_t> cnt(cells);
  if (count_out) std::fill(count_out, count_out + cells, (int64_t)0);
  for (size_t q = 0; q < k; ++q) {
    const size_t i0 = q * chunk, n = N ? std::min(chunk, N - i0) : 0;
    if (n) {
      HIPCHK(hipMemcpy(dct, ct + i0 * W, n * W * 4, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(dexp, exp + i0, n * 4, hipMemcpyHostToDevice));
      // (the last row of a strided matrix ends after its F elements)
      HIPCHK(hipMemcpy(dbins, (const char*)bins + i0 * bin_stride * bsz, ((n - 1) * bin_stride + F) * bsz, hipMemcpyHostToDevice));
      if (node) HIPCHK(hipMemcpy(dnode, node + i0, n * 4, hipMemcpyHostToDevice));
    }
    rc = pai_histogram_dev(c, dct, dexp, n, bin_dtype, dbins, F, bin_stride, dnode, nodes, B, dpart + q * cells * W, dpexp + q * cells,
                           dcnt, nullptr);
    if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    if (count_out) {
      HIPCHK(hipMemcpy(cnt.data(), dcnt, cells * 8, hipMemcpyDeviceToHost));
      for (size_t s = 0; s < cells; ++s) count_out[s] += cnt[s];
    }
  }
  if (k > 1) {
    if ((rc = add_dev(c, dpart, dpexp, (int)k, (long long)cells, dout, dexo, nullptr))) return rc;
    HIPCHK(hipDeviceSynchronize());
  }
  HIPCHK(hipMemcpy(ct_out, dout, cells * W * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(exp_out, dexo, cells * 4, hipMemcpyDeviceToHost));
  return 0;
}

// ------------------------------------------------------------------ sparse histograms (kernels_shist.hpp)
// The bin matrix is CSR. Step one (shist_slots_dev) is the histogram above over the STORED entries: every (node,
// feature) has B + 1 slots (the bins, and one for stored missing values), entries at the feature's default bin are
// skipped, and the pseudo feature F lists all samples of every node, so that its slot 0 sums to T_v. The member lists
// go through hist_lists_dev, so runs, feature blocks and the closing segmented add are the dense call's. Step two
// (shist_finish_dev) works on the slot sums alone: S_{v,f} is one k_hist_acc run over the pair's non-empty slots but the
// default one, the S values are inverted by the batch inversion of pai_mul, and ONE 2-way gather k_add writes every
// cell of the output: (slot, -) for the other cells, (T_v, inv S) for a default cell, (T_v, -) where nothing is
// stored beside it, (-, -) for an empty cell. The slot sums and T_v are exact residues at their largest exponent, so the bits
// of step two depend on nothing in step one but the matrix; the host variant combines its chunks' slot sums first.
static size_t shist_slots(size_t nodes, size_t F, size_t B) { return nodes * (F + 1) * (B + 1); }

static int shist_check(const void* ct, const void* exp, size_t N, const void* indptr, int bin_dtype, size_t F, const void* default_bin,
                       const int32_t* node, size_t nodes, size_t B, const void* ct_out, const void* exp_out, const char* who) {
  const std::string w(who);
  if ((N && (!ct || !exp)) || !indptr || !default_bin || !ct_out || !exp_out) return fail(PAI_ERR_ARG, w + ": null pointer");
  if (bin_dtype != PAI_BIN_U8 && bin_dtype != PAI_BIN_U16) return fail(PAI_ERR_ARG, w + ": bin_dtype must be PAI_BIN_U8 or PAI_BIN_U16");
  if (F == 0) return fail(PAI_ERR_ARG, w + ": F must be at least 1");
  if (B == 0 || B > (bin_dtype == PAI_BIN_U8 ? (size_t)256 : (size_t)65536)) return fail(PAI_ERR_ARG, w + ": B out of range for the bin type");
  if (nodes == 0 || (!node && nodes != 1)) return fail(PAI_ERR_ARG, w + ": nodes must be >= 1, and 1 without node ids");
  if (nodes > HIST_MAX_CELLS || F > HIST_MAX_CELLS || nodes * F > HIST_MAX_CELLS || nodes * F * B > HIST_MAX_CELLS)
    return fail(PAI_ERR_ARG, w + ": more than 2^24 cells");
  if (N >= ((size_t)1 << 31)) return fail(PAI_ERR_ARG, w + ": N must be below 2^31");
  return 0;
}

// d_sct / d_sexp [shist_slots]: the slot sums; their member counts stay in c->hist.cnt
static int shist_slots_dev(pai_ctx* c, const char* who, const uint32_t* d_ct, const int32_t* d_exp, size_t N, const int64_t* d_indptr,
                           const int32_t* d_indices, int bin_dtype, const void* d_data, size_t F, const int32_t* d_default,
                           const int32_t* d_node, size_t nodes, size_t B, uint32_t* d_sct, int32_t* d_sexp, hipStream_t st) {
  const std::string w(who);
  auto& h = c->hist;
  int rc = ensure_buf(&c->d_shisterr, &c->shisterr_bytes, 16);
  if (rc) return rc;
  unsigned* d_err = (unsigned*)c->d_shisterr;
  HIPCHK(hipMemsetAsync(d_err, 0, 4, st));
  static_assert(sizeof(long long) == sizeof(int64_t), "indptr");
  HIPCHK(shist_indptr_launch((const long long*)d_indptr, (long long)N, d_err, c->cus, st));
  HIPCHK(hipMemcpyAsync(&h.nnz, d_indptr + N, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&h.err, d_err, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (h.err) return fail(PAI_ERR_ARG, w + ": indptr must start at 0 and must not decrease");
  if (h.nnz < 0 || h.nnz >= (1ll << 31)) return fail(PAI_ERR_ARG, w + ": nnz must be below 2^31");
  if (h.nnz && (!d_indices || !d_data)) return fail(PAI_ERR_ARG, w + ": null pointer");
  SHistParams sp{};
  sp.indptr = (const long long*)d_indptr;
  sp.indices = d_indices;
  sp.data = d_data;
  sp.bin_u16 = bin_dtype == PAI_BIN_U16 ? 1 : 0;
  sp.default_bin = d_default;
  sp.node = d_node;
  sp.nodes = (int)nodes;
  sp.B = (int)B;
  sp.N = (long long)N;
  sp.F = (long long)F;
  sp.nnz = h.nnz;
  sp.err = d_err;
  auto count = [&](unsigned long long* d_cnt) -> int {
    sp.count = d_cnt;
    sp.f0 = 0;
    sp.f1 = (long long)F + 1;
    HIPCHK(shist_count_launch(sp, c->cus, st));
    HIPCHK(hipMemcpyAsync(&h.err, d_err, 4, hipMemcpyDeviceToHost, st));
    return 0;
  };
  auto counted = [&]() -> int {
    if (h.err & SHIST_ERR_INDEX) return fail(PAI_ERR_ARG, w + ": index outside [0, F)");
    if (h.err & SHIST_ERR_ORDER) return fail(PAI_ERR_ARG, w + ": the indices of a row must be strictly increasing");
    return 0;
  };
  auto scatter = [&](size_t f0, size_t f1, unsigned long long* d_cnt, const int32_t* d_off, unsigned* d_cur, int32_t* d_mem) {
    sp.count = d_cnt;
    sp.cell_off = d_off;
    sp.cursor = d_cur;
    sp.members = d_mem;
    sp.f0 = (long long)f0;
    sp.f1 = (long long)f1;
    return shist_scatter_launch(sp, c->cus, st);
  };
  return hist_lists_dev(c, w, d_ct, d_exp, N, F + 1, nodes, B + 1, count, counted, scatter, d_sct, d_sexp, nullptr, st);
}

// d_s / d_se hold the slot sums and room for nodes F more rows (the S values). cnt: members per slot, zs: default bins
// (both host memory).
static int shist_finish_dev(pai_ctx* c, const char* who, uint32_t* d_s, int32_t* d_se, const long long* cnt, const int32_t* zs, size_t F,
                            size_t nodes, size_t B, uint32_t* d_out, int32_t* d_exp_out, int64_t* d_count_out, hipStream_t st) {
  const size_t F1 = F + 1, B1 = B + 1, slots = shist_slots(nodes, F, B), cells = nodes * F * B, W = c->ct_words;
  auto& h = c->hist;
  h.sgidx.assign(cells * 2, -1ll);
  h.scount.assign(cells, 0);
  h.smem.clear();
  h.sruns.clear();
  for (size_t v = 0; v < nodes; ++v) {
    const size_t total = (v * F1 + F) * B1;
    for (size_t f = 0; f < F; ++f) {
      const size_t base = (v * F1 + f) * B1, cell0 = (v * F + f) * B;
      const bool has = zs[f] >= 0 && (size_t)zs[f] < B;
      const size_t z = has ? (size_t)zs[f] : B1;
      for (size_t b = 0; b < B; ++b) {
        if (b == z) continue;
        h.scount[cell0 + b] = cnt[base + b];
        if (cnt[base + b]) h.sgidx[2 * (cell0 + b)] = (long long)(base + b);
      }
      if (!has) continue;
      const size_t first = h.smem.size();
      long long stored = 0;
      for (size_t q = 0; q < B1; ++q)
        if (q != z && cnt[base + q]) {
          stored += cnt[base + q];
          h.smem.push_back((int32_t)(base + q));
        }
      const long long rest = cnt[total] - stored;
      if (rest < 0) return fail(PAI_ERR_ARG, std::string(who) + ": a node holds more stored entries of a feature than samples");
      h.scount[cell0 + z] = rest;
      if (rest == 0 || stored == 0) h.smem.resize(first);        // an empty default cell, or T_v itself: no S
      if (rest == 0) continue;
      h.sgidx[2 * (cell0 + z)] = (long long)total;
      if (stored) {
        h.sgidx[2 * (cell0 + z) + 1] = (long long)(slots + h.sruns.size());
        h.sruns.push_back(make_int2((int)first, (int)(h.smem.size() - first)));
      }
    }
  }
  const size_t pairs = h.sruns.size(), o_runs = align16(h.smem.size() * 4), o_g = align16(o_runs + pairs * 8);
  int rc = ensure_buf(&c->d_histwork, &c->histwork_bytes, o_g + cells * 16);
  if (rc) return rc;
  int32_t* d_mem = (int32_t*)c->d_histwork;
  int2* d_runs = (int2*)((char*)c->d_histwork + o_runs);
  long long* d_g = (long long*)((char*)c->d_histwork + o_g);
  HIPCHK(hipMemcpyAsync(d_g, h.sgidx.data(), cells * 16, hipMemcpyHostToDevice, st));
  if (pairs) {
    HIPCHK(hipMemcpyAsync(d_mem, h.smem.data(), h.smem.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_runs, h.sruns.data(), pairs * 8, hipMemcpyHostToDevice, st));
    HistAccParams ap{};
    ap.cts = d_s;
    ap.exps = d_se;
    ap.members = d_mem;
    ap.runs = d_runs;
    ap.nruns = (long long)pairs;
    ap.out = d_s + slots * W;
    ap.out_exp = d_se + slots;
    ap.N = c->d_N;
    ap.RS = c->d_RS;
    ap.mprime = c->mprime_N;
    ap.ct_words = c->ct_words;
    HIPCHK(hist_acc_launch(c->tpi_e, ap, c->cus, st));
    if ((rc = batch_invert(c, d_s + slots * W, nullptr, (long long)pairs, st))) return rc;
  }
  if ((rc = run_add(c, add_params(d_s, d_se, 2, (long long)cells, d_out, d_exp_out, d_g), st))) return rc;
  if (d_count_out) HIPCHK(hipMemcpyAsync(d_count_out, h.scount.data(), cells * 8, hipMemcpyHostToDevice, st));
  return 0;
}

int pai_histogram_sparse_dev(pai_ctx* c, const uint32_t* d_ct, const int32_t* d_exp, size_t N, const int64_t* d_indptr,
                             const int32_t* d_indices, int bin_dtype, const void* d_data, size_t F, const int32_t* d_default_bin,
                             const int32_t* d_node, size_t nodes, size_t B, uint32_t* d_out, int32_t* d_exp_out,
                             int64_t* d_count_out, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  const char* who = "pai_histogram_sparse_dev";
  int rc = shist_check(d_ct, d_exp, N, d_indptr, bin_dtype, F, d_default_bin, d_node, nodes, B, d_out, d_exp_out, who);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t W = c->ct_words, rows = shist_slots(nodes, F, B) + nodes * F, o_exp = align16(rows * W * 4);
  if ((rc = ensure_buf(&c->d_shist, &c->shist_bytes, o_exp + rows * 4))) return rc;
  uint32_t* d_s = (uint32_t*)c->d_shist;
  int32_t* d_se = (int32_t*)((char*)c->d_shist + o_exp);
  c->hist.zs.assign(F, 0);
  HIPCHK(hipMemcpyAsync(c->hist.zs.data(), d_default_bin, F * 4, hipMemcpyDeviceToHost, st));   // (read after the next synchronisation)
  if ((rc = shist_slots_dev(c, who, d_ct, d_exp, N, d_indptr, d_indices, bin_dtype, d_data, F, d_default_bin, d_node, nodes, B, d_s,
                            d_se, st)))
    return rc;
  return shist_finish_dev(c, who, d_s, d_se, c->hist.cnt.data(), c->hist.zs.data(), F, nodes, B, d_out, d_exp_out, d_count_out, st);
}

int pai_histogram_sparse(pai_ctx* c, const uint32_t* ct, const int32_t* exp, size_t N, const int64_t* indptr, const int32_t* indices,
                         int bin_dtype, const void* data, size_t F, const int32_t* default_bin, const int32_t* node, size_t nodes,
                         size_t B, uint32_t* ct_out, int32_t* exp_out, int64_t* count_out) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  const char* who = "pai_histogram_sparse";
  int rc = shist_check(ct, exp, N, indptr, bin_dtype, F, default_bin, node, nodes, B, ct_out, exp_out, who);
  if (rc) return rc;
  // (the offsets cut host arrays below, so they are checked here; the indices are checked on the device)
  if (indptr[0] != 0) return fail(PAI_ERR_ARG, std::string(who) + ": indptr must start at 0 and must not decrease");
  for (size_t i = 0; i < N; ++i)
    if (indptr[i + 1] < indptr[i]) return fail(PAI_ERR_ARG, std::string(who) + ": indptr must start at 0 and must not decrease");
  if (indptr[N] >= (1ll << 31)) return fail(PAI_ERR_ARG, std::string(who) + ": nnz must be below 2^31");
  if (indptr[N] && (!indices || !data)) return fail(PAI_ERR_ARG, std::string(who) + ": null pointer");
  HIPCHK(hipSetDevice(c->device));
  const size_t W = c->ct_words, slots = shist_slots(nodes, F, B), cells = nodes * F * B, rows = slots + nodes * F,
               bsz = bin_dtype == PAI_BIN_U16 ? 2 : 1;
  // chunks of samples as in pai_histogram; their slot sums [chunk][slots] are the operands of one k-way add
  size_t chunk = HIST_HOST_CHUNK;
  if (const char* e = xcheck_env("FLEXPAI_HIST_CHUNK")) {           // test build: chunks at small shapes
    const unsigned long long v = strtoull(e, nullptr, 10);
    if (v > 0) chunk = (size_t)v;
  }
  const size_t kmax = std::max<size_t>(HIST_HOST_PART_BYTES / (slots * W * 4), 1);
  if ((N + chunk - 1) / chunk > kmax) chunk = (N + kmax - 1) / kmax;
  const size_t k = std::max<size_t>((N + chunk - 1) / chunk, 1), nc = std::min(chunk, std::max<size_t>(N, 1));
  size_t ne = 0;
  for (size_t i0 = 0; i0 < N; i0 += chunk) ne = std::max(ne, (size_t)(indptr[std::min(N, i0 + chunk)] - indptr[i0]));
  DevScope ds;
  uint32_t* dct = ds.alloc<uint32_t>(nc * W);
  int32_t* dexp = ds.alloc<int32_t>(nc);
  int64_t* dptr = ds.alloc<int64_t>(nc + 1);
  int32_t* dind = ds.alloc<int32_t>(ne);
  uint8_t* ddata = ds.alloc<uint8_t>(ne * bsz);
  int32_t* ddef = ds.alloc<int32_t>(F);
  int32_t* dnode = node ? ds.alloc<int32_t>(nc) : nullptr;
  // (k == 1: the chunk's slot sums are the finish step's buffer, with the S rows after them)
  uint32_t* dpart = ds.alloc<uint32_t>(k > 1 ? k * slots * W : rows * W);
  int32_t* dpexp = ds.alloc<int32_t>(k > 1 ? k * slots : rows);
  uint32_t* dsum = k > 1 ? ds.alloc<uint32_t>(rows * W) : dpart;
  int32_t* dsexp = k > 1 ? ds.alloc<int32_t>(rows) : dpexp;
  uint32_t* dout = ds.alloc<uint32_t>(cells * W);
  int32_t* dexo = ds.alloc<int32_t>(cells);
  int64_t* dcnt = ds.alloc<int64_t>(cells);
  if (!dct || !dexp || !dptr || !dind || !ddata || !ddef || (node && !dnode) || !dpart || !dpexp || !dsum || !dsexp || !dout || !dexo ||
      !dcnt)
    return fail(PAI_ERR_HIP, std::string(who) + ": device allocation failed");
  HIPCHK(hipMemcpy(ddef, default_bin, F * 4, hipMemcpyHostToDevice));
  std::vector<long long> cnt(slots, 0);
  std::vector<int64_t> ptr(nc + 1);
  for (size_t q = 0; q < k; ++q) {
    const size_t i0 = q * chunk, n = N ? std::min(chunk, N - i0) : 0;
    const int64_t e0 = indptr[i0];
    const size_t m = (size_t)(indptr[i0 + n] - e0);
    for (size_t i = 0; i <= n; ++i) ptr[i] = indptr[i0 + i] - e0;
    HIPCHK(hipMemcpy(dptr, ptr.data(), (n + 1) * 8, hipMemcpyHostToDevice));
    if (n) {
      HIPCHK(hipMemcpy(dct, ct + i0 * W, n * W * 4, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(dexp, exp + i0, n * 4, hipMemcpyHostToDevice));
      if (node) HIPCHK(hipMemcpy(dnode, node + i0, n * 4, hipMemcpyHostToDevice));
    }
    if (m) {
      HIPCHK(hipMemcpy(dind, indices + e0, m * 4, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(ddata, (const char*)data + (size_t)e0 * bsz, m * bsz, hipMemcpyHostToDevice));
    }
    if ((rc = shist_slots_dev(c, who, dct, dexp, n, dptr, dind, bin_dtype, ddata, F, ddef, dnode, nodes, B, dpart + q * slots * W,
                              dpexp + q * slots, nullptr)))
      return rc;
    HIPCHK(hipDeviceSynchronize());
    for (size_t s = 0; s < slots; ++s) cnt[s] += c->hist.cnt[s];
  }
  if (k > 1 && (rc = add_dev(c, dpart, dpexp, (int)k, (long long)slots, dsum, dsexp, nullptr))) return rc;
  if ((rc = shist_finish_dev(c, who, dsum, dsexp, cnt.data(), default_bin, F, nodes, B, dout, dexo, dcnt, nullptr))) return rc;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(ct_out, dout, cells * W * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(exp_out, dexo, cells * 4, hipMemcpyDeviceToHost));
  if (count_out) HIPCHK(hipMemcpy(count_out, dcnt, cells * 8, hipMemcpyDeviceToHost));
  return 0;
}

// ------------------------------------------------------------------ prefix sums (kernels_scan.hpp)
// Row chains: one k_scan lane group per (o, i) row. Blocked: the rows are cut into tiles of T; k_scan writes the tiles'
// totals, the totals [outer][tiles][inner] are scanned by the same routine (recursively), and k_scan runs per tile from
// the scanned total of the tiles before it. The automatic T gives the chip's resident lane groups (scan_slots) one
// tile each, but no tile shorter than SCAN_TILE_FLOOR: a tile costs its total (one product per element, against two
// for the chain) and a carry product, and short tiles deepen the recursion.
// SCAN_TILE_FLOOR = 8, from the forced tiles of tools/cumsum_ab.py (profiles/cumsum_ab.json), at
// 1024 / 2048 bits: one vector of 2^18 elements takes 2.90 / 5.50 ms in tiles of 4, 3.31 / 5.77 in tiles of 8, 4.64 / 7.33
// in tiles of 16, 6.86 / 10.72 in tiles of 32 and 11.20 / 17.54 in tiles of 64; 8192 rows of 32 take 1.00 / 2.47 ms in
// tiles of 4, 0.86 / 1.92 in tiles of 8, 1.30 / 2.05 in tiles of 16 and 1.36 / 2.16 as row chains; 1024 rows of 256 take
// 1.39 / 3.25, 1.44 / 2.90 and 1.88 / 3.04 ms in tiles of 4, 8 and 16. Tiles of 4 win by 4 to 12 % on the vector and on 1024 x 256 at
// 1024 bits and lose by 12 to 29 % on the rows of 32 at both sizes and on 1024 x 256 at 2048 bits.
constexpr long long SCAN_TILE_FLOOR = 8;

static long long scan_tile_for(const pai_ctx* c, long long rows, long long L, long long slots) {
  if (c->scan_tile > 0) return std::min<long long>(c->scan_tile, L);
  const long long want = (slots + rows - 1) / rows;          // tiles per row that fill the chip once
  if (want <= 1) return L;
  return std::min(L, std::max(SCAN_TILE_FLOOR, (L + want - 1) / want));
}

// bytes of d_scan that a scan of [outer][L][inner] needs below itself: per level the tiles' totals and their scan
static size_t scan_scratch(const pai_ctx* c, long long outer, long long L, long long inner, long long slots) {
  size_t total = 0;
  for (;;) {
    const long long T = scan_tile_for(c, outer * inner, L, slots);
    if (T >= L || T < 2) return total;
    const long long tiles = (L + T - 1) / T;
    const size_t n = (size_t)(outer * tiles * inner);
    total += 2 * (align16(n * c->ct_words * 4) + align16(n * 4));
    L = tiles;
  }
}

static int scan_level(pai_ctx* c, const uint32_t* ct, const int32_t* exp, long long outer, long long L, long long inner, int reverse,
                      uint32_t* out, int32_t* exp_out, char* scratch, long long slots, int depth, hipStream_t st) {
  ScanParams p{};
  p.ct = ct;
  p.exp = exp;
  p.outer = outer;
  p.L = L;
  p.inner = inner;
  p.reverse = reverse;
  p.N = c->d_N;
  p.R2 = c->d_R2;
  p.oneR = c->d_oneR;
  p.RS = c->d_RS;
  p.mprime = c->mprime_N;
  p.ct_words = c->ct_words;
  long long T = scan_tile_for(c, outer * inner, L, slots);
  if (T < 2) T = L;                                          // tiles of one element would never shorten the totals
  if (T >= L) {
    p.T = L;
    p.tiles = 1;
    p.emit_all = 1;
    p.out = out;
    p.out_exp = exp_out;
    if (depth == 0) c->scan_path = 1;
    HIPCHK(scan_launch(c->tpi_e, p, c->cus, st));
    return 0;
  }
  if (depth == 0) c->scan_path = 2;
  const long long tiles = (L + T - 1) / T;
  const size_t n = (size_t)(outer * tiles * inner), wb = align16(n * c->ct_words * 4), eb = align16(n * 4);
  uint32_t* tot = (uint32_t*)scratch;
  int32_t* tot_e = (int32_t*)(scratch + wb);
  uint32_t* car = (uint32_t*)(scratch + wb + eb);
  int32_t* car_e = (int32_t*)(scratch + 2 * wb + eb);
  p.T = T;
  p.tiles = tiles;
  p.emit_all = 0;
  p.out = tot;
  p.out_exp = tot_e;
  HIPCHK(scan_launch(c->tpi_e, p, c->cus, st));
  int rc = scan_level(c, tot, tot_e, outer, tiles, inner, reverse, car, car_e, scratch + 2 * (wb + eb), slots, depth + 1, st);
  if (rc) return rc;
  p.emit_all = 1;
  p.carry = car;
  p.carry_exp = car_e;
  p.out = out;
  p.out_exp = exp_out;
  HIPCHK(scan_launch(c->tpi_e, p, c->cus, st));
  return 0;
}

static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

// 1: nothing to do, 0: go on, < 0: error
static int scan_check(const pai_ctx* c, const void* ct, const void* exp, size_t outer, size_t L, size_t inner, int flags,
                      const void* ct_out, const void* exp_out, const char* who) {
  const std::string w(who);
  if (flags & ~PAI_SCAN_REVERSE) return fail(PAI_ERR_ARG, w + ": unknown flag bits");
  if (outer == 0 || L == 0 || inner == 0) return 1;
  if (!ct || !exp || !ct_out || !exp_out) return fail(PAI_ERR_ARG, w + ": null pointer");
  const size_t lim = (size_t)1 << 31;
  if (outer >= lim || L >= lim || inner >= lim || outer * L >= lim || outer * L * inner >= lim)
    return fail(PAI_ERR_ARG, w + ": outer L inner must be below 2^31");
  const size_t n = outer * L * inner, cb = n * c->ct_words * 4, eb = n * 4;
  if (ranges_overlap(ct, cb, ct_out, cb) || ranges_overlap(exp, eb, exp_out, eb) || ranges_overlap(ct, cb, exp_out, eb) ||
      ranges_overlap(exp, eb, ct_out, cb))
    return fail(PAI_ERR_ARG, w + ": the output overlaps the input");
  return 0;
}

int pai_cumsum_dev(pai_ctx* c, const uint32_t* d_ct, const int32_t* d_exp, size_t outer, size_t L, size_t inner, int flags,
                   uint32_t* d_out, int32_t* d_exp_out, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  int rc = scan_check(c, d_ct, d_exp, outer, L, inner, flags, d_out, d_exp_out, "pai_cumsum_dev");
  if (rc) return rc < 0 ? rc : 0;
  HIPCHK(hipSetDevice(c->device));
  const long long slots = scan_slots(c->tpi_e, c->cus);
  if (slots <= 0) return fail(PAI_ERR_KEY, "unsupported group size");
  if ((rc = ensure_buf(&c->d_scan, &c->scan_bytes, scan_scratch(c, (long long)outer, (long long)L, (long long)inner, slots)))) return rc;
  return scan_level(c, d_ct, d_exp, (long long)outer, (long long)L, (long long)inner, (flags & PAI_SCAN_REVERSE) ? 1 : 0, d_out,
                    d_exp_out, (char*)c->d_scan, slots, 0, (hipStream_t)stream);
}

// Slices of whole `outer` indices of at most SCAN_HOST_BYTES of ciphertext each (one index at least): every (o, i) row
// lies in one slice, so the slices change no bits.
constexpr size_t SCAN_HOST_BYTES = (size_t)1 << 30;

int pai_cumsum(pai_ctx* c, const uint32_t* ct, const int32_t* exp, size_t outer, size_t L, size_t inner, int flags,
               uint32_t* ct_out, int32_t* exp_out) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  int rc = scan_check(c, ct, exp, outer, L, inner, flags, ct_out, exp_out, "pai_cumsum");
  if (rc) return rc < 0 ? rc : 0;
  HIPCHK(hipSetDevice(c->device));
  const size_t W = c->ct_words, row = L * inner;
  const size_t per = std::min(outer, std::max<size_t>(SCAN_HOST_BYTES / (row * W * 4), 1));
  DevScope ds;
  uint32_t* din = ds.alloc<uint32_t>(per * row * W);
  int32_t* dein = ds.alloc<int32_t>(per * row);
  uint32_t* dout = ds.alloc<uint32_t>(per * row * W);
  int32_t* deout = ds.alloc<int32_t>(per * row);
  if (!din || !dein || !dout || !deout) return fail(PAI_ERR_HIP, "pai_cumsum: device allocation failed");
  for (size_t o0 = 0; o0 < outer; o0 += per) {
    const size_t no = std::min(per, outer - o0), n = no * row;
    HIPCHK(hipMemcpy(din, ct + o0 * row * W, n * W * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dein, exp + o0 * row, n * 4, hipMemcpyHostToDevice));
    if ((rc = pai_cumsum_dev(c, din, dein, no, L, inner, flags, dout, deout, nullptr))) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(ct_out + o0 * row * W, dout, n * W * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(exp_out + o0 * row, deout, n * 4, hipMemcpyDeviceToHost));
  }
  return 0;
}

int pai_matmul(pai_ctx* c, const uint32_t* ct, const int32_t* exp, size_t m, size_t K, int dtype, const void* x,
               size_t d, uint32_t* ct_out, int32_t* exp_out) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (m == 0 || d == 0) return 0;
  if (K == 0 || !ct || !exp || !x || !ct_out || !exp_out) return fail(PAI_ERR_ARG, "pai_matmul: bad arguments");
  HIPCHK(hipSetDevice(c->device));
  const size_t W = c->ct_words, esz = dtype == PAI_F32 ? 4 : 8;
  DevScope ds;
  uint32_t* dct = ds.alloc<uint32_t>(m * K * W);
  int32_t* dexp = ds.alloc<int32_t>(m * K);
  void* dx = ds.alloc<uint8_t>(K * d * esz);
  uint32_t* dout = ds.alloc<uint32_t>(m * d * W);
  int32_t* dexo = ds.alloc<int32_t>(m * d);
  if (!dct || !dexp || !dx || !dout || !dexo) return fail(PAI_ERR_HIP, "pai_matmul: device allocation failed");
  HIPCHK(hipMemcpy(dct, ct, m * K * W * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dexp, exp, m * K * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dx, x, K * d * esz, hipMemcpyHostToDevice));
  int rc = pai_matmul_dev(c, dct, dexp, m, K, dtype, dx, d, dout, dexo, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(ct_out, dout, m * d * W * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(exp_out, dexo, m * d * 4, hipMemcpyDeviceToHost));
  return 0;
}

int pai_segment_dot(pai_ctx* c, const uint32_t* ct, const int32_t* exp, size_t N, const int64_t* index,
                    const int64_t* seg_off, size_t nseg, int dtype, const void* x, uint32_t* ct_out, int32_t* exp_out,
                    int32_t* status_out) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (nseg == 0) return 0;
  if ((N && (!ct || !exp)) || !seg_off || !ct_out || !exp_out || dtype < 0 || dtype > 2 || seg_off[0] != 0 ||
      seg_off[nseg] < 0 || (seg_off[nseg] > 0 && !x))
    return fail(PAI_ERR_ARG, "pai_segment_dot: bad arguments");
  HIPCHK(hipSetDevice(c->device));
  const size_t W = c->ct_words, esz = dtype == PAI_F32 ? 4 : 8, nnz = (size_t)seg_off[nseg];
  DevScope ds;
  uint32_t* dct = ds.alloc<uint32_t>(N * W);
  int32_t* dexp = ds.alloc<int32_t>(N);
  void* dx = ds.alloc<uint8_t>(nnz * esz);
  uint32_t* dout = ds.alloc<uint32_t>(nseg * W);
  int32_t* dexo = ds.alloc<int32_t>(nseg);
  int32_t* dst = ds.alloc<int32_t>(nnz);
  if (!dct || !dexp || !dx || !dout || !dexo || !dst) return fail(PAI_ERR_HIP, "pai_segment_dot: device allocation failed");
  if (N) {
    HIPCHK(hipMemcpy(dct, ct, N * W * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dexp, exp, N * 4, hipMemcpyHostToDevice));
  }
  if (nnz) HIPCHK(hipMemcpy(dx, x, nnz * esz, hipMemcpyHostToDevice));
  int rc = pai_segment_dot_dev(c, dct, dexp, N, index, seg_off, nseg, dtype, dx, dout, dexo, dst, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(ct_out, dout, nseg * W * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(exp_out, dexo, nseg * 4, hipMemcpyDeviceToHost));
  if (status_out && nnz) HIPCHK(hipMemcpy(status_out, dst, nnz * 4, hipMemcpyDeviceToHost));
  return 0;
}

// ------------------------------------------------------------------ host-buffer entry points
// The operands cross PCIe in chunks that overlap the kernels: outputs of chunk i are copied to the
// caller while chunk i+1 computes (encrypt), inputs of chunk i+1 are copied while chunk i computes
// (decrypt, add). Ciphertexts do not depend on the chunking (the device RNG is keyed by the global
// element index). Device copies live in one buffer kept by the context (grown on demand).
constexpr size_t HOST_CHUNK_MIN = (size_t)1 << 17;   // elements: large enough to fill the chip per chunk
constexpr int HOST_CHUNKS_MAX = 16;
constexpr size_t PIN_SLOT_MAX = (size_t)64 << 20;     // bytes per pinned staging slot (two slots)

// Chunking for N elements moving stage_per_elem bytes each through the pinned slots; grows the
// context's device buffer to dev_bytes, the pinned slots and the per-chunk events.
static int host_pipe(pai_ctx* c, size_t N, size_t dev_bytes, size_t stage_per_elem, size_t* chunk, int* nch) {
  if (!c->s_comp) HIPCHK(hipStreamCreateWithFlags(&c->s_comp, hipStreamNonBlocking));
  if (!c->s_copy) HIPCHK(hipStreamCreateWithFlags(&c->s_copy, hipStreamNonBlocking));
  size_t k = std::max<size_t>(1, std::min<size_t>(HOST_CHUNKS_MAX, N / HOST_CHUNK_MIN));
  k = std::max(k, (N * stage_per_elem + PIN_SLOT_MAX - 1) / PIN_SLOT_MAX);
  *chunk = (N + k - 1) / k;
  *nch = (int)((N + *chunk - 1) / *chunk);
  for (auto* v : {&c->hev, &c->pev, &c->oev})
    while (v->size() < (size_t)*nch) {
      hipEvent_t e;
      HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      v->push_back(e);
    }
  const size_t slot = *chunk * stage_per_elem;
  if (slot > c->pin_bytes) {
    for (void*& p : c->h_pin) {
      if (p) HIPCHK(hipHostFree(p));
      p = nullptr;
    }
    c->pin_bytes = 0;
    for (void*& p : c->h_pin) HIPCHK(hipHostMalloc(&p, slot, hipHostMallocDefault));
    c->pin_bytes = slot;
  }
  return ensure_buf(&c->d_hostio, &c->hostio_bytes, dev_bytes);
}

// memcpy between the pinned slots and caller memory on several host threads (a single thread moves
// ~10 GB/s, below the PCIe rate).
static void par_copy(void* dst, const void* src, size_t bytes) {
  const size_t hw = std::max(1u, std::thread::hardware_concurrency());
  const size_t T = bytes < ((size_t)4 << 20) ? 1 : std::min<size_t>(16, hw);
  if (T == 1) {
    std::memcpy(dst, src, bytes);
    return;
  }
  const size_t part = ((bytes + T - 1) / T + 4095) & ~(size_t)4095;
  std::vector<std::thread> th;
  for (size_t t = 0; t < T && t * part < bytes; ++t)
    th.emplace_back([=] { std::memcpy((char*)dst + t * part, (const char*)src + t * part, std::min(part, bytes - t * part)); });
  for (auto& x : th) x.join();
}

// Carves typed regions out of the context's host-io buffer (256-byte aligned).
struct Carve {
  char* base;
  size_t off = 0;
  template <typename T>
  T* take(size_t n) {
    T* p = (T*)(base + off);
    off = (off + std::max<size_t>(n, 1) * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
};
static size_t carve_bytes(std::initializer_list<size_t> sizes) {
  size_t t = 0;
  for (size_t b : sizes) t += (std::max<size_t>(b, 1) + 255) & ~(size_t)255;
  return t;
}

// Scope of one host-buffer call (pai_encrypt / pai_add / pai_decrypt): the stage timing is reset once and
// then spans every chunk's *_dev call; the fixed-base decision of the call is dropped at exit.
struct HostCall {
  pai_ctx* c;
  explicit HostCall(pai_ctx* ctx) : c(ctx) {
    stage_reset(c);
    c->stage_keep = true;
  }
  ~HostCall() {
    c->stage_keep = false;
    c->fb_call = 0;
    c->pfb_call = 0;
  }
};

int pai_encrypt(pai_ctx* c, int dtype, const void* x, size_t N, int exp_mode, int32_t fixed_exp, int obf_mode,
                const uint8_t* r_le, size_t r_stride_bytes, size_t r_bytes, const uint8_t* rng_key32,
                uint64_t index_base, uint32_t* ct_out, int32_t* exp_out, int32_t* status_out) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (N == 0) return 0;
  if (!x || !ct_out || !exp_out) return fail(PAI_ERR_ARG, "pai_encrypt: null buffer");
  if (obf_mode == PAI_OBF_GIVEN && (!r_le || r_bytes == 0)) return fail(PAI_ERR_ARG, "pai_encrypt: r required");
  if (obf_mode == PAI_OBF_POOL) {   // the whole call or nothing: its chunks then take their entries in order
    if (dtype < 0 || dtype > 2) return fail(PAI_ERR_ARG, "pai_encrypt: bad dtype");
    const int prc = pool_check_take(c, N, "pai_encrypt");
    if (prc) return prc;
  }
  HIPCHK(hipSetDevice(c->device));
  const size_t esz = dtype == PAI_F32 ? 4 : 8, W = c->ct_words;
  const size_t r_words = obf_mode == PAI_OBF_GIVEN ? (r_bytes + 3) / 4 : 0;
  const size_t r_cnt = obf_mode == PAI_OBF_GIVEN ? (r_stride_bytes ? N : 1) : 0;
  size_t CH;
  int nch, rc;
  if ((rc = host_pipe(c, N, carve_bytes({N * esz, N * W * 4, N * 4, N * 4, r_cnt * r_words * 4}), W * 4, &CH, &nch)))
    return rc;
  Carve cv{(char*)c->d_hostio};
  void* dx = cv.take<uint8_t>(N * esz);
  uint32_t* dct = cv.take<uint32_t>(N * W);
  int32_t* dexp = cv.take<int32_t>(N);
  int32_t* dst = cv.take<int32_t>(N);
  uint32_t* dr = cv.take<uint32_t>(r_cnt * r_words);
  hipStream_t sc = c->s_comp, sy = c->s_copy;
  HIPCHK(hipMemcpyAsync(dx, x, N * esz, hipMemcpyHostToDevice, sc));
  if (r_cnt) {
    std::vector<uint32_t> hr(r_cnt * r_words, 0);
    for (size_t i = 0; i < r_cnt; ++i) std::memcpy(&hr[i * r_words], r_le + i * r_stride_bytes, r_bytes);
    HIPCHK(hipMemcpyAsync(dr, hr.data(), hr.size() * 4, hipMemcpyHostToDevice, sc));
    HIPCHK(hipStreamSynchronize(sc));   // hr is released at the end of this scope
  }
  const size_t r_stride_words = r_stride_bytes ? r_words : 0;
  // one fixed-base decision and one stage-timing record for the whole call: the ciphertexts of a call do
  // not depend on how it is chunked
  HostCall hc(c);
  if (obf_mode == PAI_OBF_RNG) {
    const int sampler = encrypt_route(route_facts(c), obf_mode, (long long)N, rng_stream_words(c)).sampler;
    if (sampler == PAI_SAMPLER_KEY) c->fb_call = fb_wanted(c, (long long)N) ? 1 : -1;
    // not through the route: a key holder's call counts towards the key holder's break-even here with the fixed base
    // switched off too, which the device entry does not do (pai_ctx_fixed_base_policy's `seen` reports it)
    else if ((c->crt_ok || c->fbg_ok) && c->crt_enabled) c->fb_call = fb_wanted(c, (long long)N) ? 1 : -1;
    else if (sampler == PAI_SAMPLER_PUBLIC) c->pfb_call = pfb_wanted(c, (long long)N) ? 1 : -1;
  }
  // every chunk's kernels are queued first; the copy stream then drains chunk i while i+1.. compute
  for (int i = 0; i < nch; ++i) {
    const size_t off = (size_t)i * CH, n = std::min(CH, N - off);
    rc = pai_encrypt_dev(c, dtype, (const char*)dx + off * esz, n, exp_mode, fixed_exp, obf_mode,
                         dr ? dr + off * r_stride_words : nullptr, r_stride_words, r_words, rng_key32,
                         index_base + off, dct + off * W, dexp + off, dst + off, sc);
    if (rc) {
      (void)hipStreamSynchronize(sc);
      return rc;
    }
    HIPCHK(hipEventRecord(c->hev[i], sc));
  }
  // ciphertext words: device -> pinned slot (i & 1) on the copy stream, then the host threads move the
  // slot into the caller's buffer while chunk i+1 crosses PCIe and later chunks compute
  auto d2h = [&](int i) -> int {
    const size_t off = (size_t)i * CH, n = std::min(CH, N - off);
    HIPCHK(hipStreamWaitEvent(sy, c->hev[i], 0));
    HIPCHK(hipMemcpyAsync(c->h_pin[i & 1], dct + off * W, n * W * 4, hipMemcpyDeviceToHost, sy));
    HIPCHK(hipEventRecord(c->pev[i], sy));
    return 0;
  };
  if ((rc = d2h(0))) return rc;
  for (int i = 0; i < nch; ++i) {
    if (i + 1 < nch && (rc = d2h(i + 1))) return rc;   // its slot's previous chunk (i - 1) is consumed
    const size_t off = (size_t)i * CH, n = std::min(CH, N - off);
    HIPCHK(hipEventSynchronize(c->pev[i]));
    par_copy(ct_out + off * W, c->h_pin[i & 1], n * W * 4);
  }
  HIPCHK(hipMemcpyAsync(exp_out, dexp, N * 4, hipMemcpyDeviceToHost, sc));
  if (status_out) HIPCHK(hipMemcpyAsync(status_out, dst, N * 4, hipMemcpyDeviceToHost, sc));
  HIPCHK(hipStreamSynchronize(sc));
  HIPCHK(hipStreamSynchronize(sy));
  return 0;
}

int pai_add(pai_ctx* c, const uint32_t* const* cts, const int32_t* const* exps, int k, size_t N, uint32_t* ct_out,
            int32_t* exp_out) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (N == 0) return 0;
  if (k < 1 || !cts || !exps || !ct_out || !exp_out) return fail(PAI_ERR_ARG, "pai_add: bad arguments");
  for (int j = 0; j < k; ++j)
    if (!cts[j] || !exps[j]) return fail(PAI_ERR_ARG, "pai_add: null operand");
  HIPCHK(hipSetDevice(c->device));
  const size_t W = c->ct_words;
  size_t CH;
  int nch, rc;
  if ((rc = host_pipe(c, N, carve_bytes({(size_t)k * N * W * 4, (size_t)k * N * 4, N * W * 4, N * 4}),
                     (size_t)k * W * 4, &CH, &nch)))
    return rc;
  Carve cv{(char*)c->d_hostio};
  // chunk i's operands are contiguous [k][n_i][W] at offset k off (the k_add layout of that chunk)
  uint32_t* dcts = cv.take<uint32_t>((size_t)k * N * W);
  int32_t* dexps = cv.take<int32_t>((size_t)k * N);
  uint32_t* dout = cv.take<uint32_t>(N * W);
  int32_t* dexp = cv.take<int32_t>(N);
  hipStream_t sc = c->s_comp, sy = c->s_copy;
  HostCall hc(c);
  for (int i = 0; i < nch; ++i) {
    const size_t off = (size_t)i * CH, n = std::min(CH, N - off);
    uint32_t* cc = dcts + (size_t)k * off * W;
    int32_t* ce = dexps + (size_t)k * off;
    // inputs of chunk i: caller -> pinned slot (host threads, while chunk i-1 computes) -> device
    if (i >= 2) HIPCHK(hipEventSynchronize(c->hev[i - 2]));   // the slot's previous upload is done
    uint32_t* slot = (uint32_t*)c->h_pin[i & 1];
    for (int j = 0; j < k; ++j) par_copy(slot + (size_t)j * n * W, cts[j] + off * W, n * W * 4);
    HIPCHK(hipMemcpyAsync(cc, slot, (size_t)k * n * W * 4, hipMemcpyHostToDevice, sy));
    for (int j = 0; j < k; ++j)
      HIPCHK(hipMemcpyAsync(ce + (size_t)j * n, exps[j] + off, n * 4, hipMemcpyHostToDevice, sy));
    HIPCHK(hipEventRecord(c->hev[i], sy));
    HIPCHK(hipStreamWaitEvent(sc, c->hev[i], 0));
    if ((rc = pai_add_dev(c, cc, ce, k, n, dout + off * W, dexp + off, sc))) {
      (void)hipStreamSynchronize(sc);
      return rc;
    }
  }
  HIPCHK(hipMemcpyAsync(ct_out, dout, N * W * 4, hipMemcpyDeviceToHost, sc));
  HIPCHK(hipMemcpyAsync(exp_out, dexp, N * 4, hipMemcpyDeviceToHost, sc));
  HIPCHK(hipStreamSynchronize(sc));
  return 0;
}

// Inputs cross host-to-device per chunk ahead of the kernels (as in pai_add), every chunk is re-randomised in place on
// the device, and the outputs drain through the two pinned slots (as in pai_encrypt) once the last upload has left them.
int pai_obfuscate(pai_ctx* c, const uint32_t* ct, size_t N, int obf_mode, const uint8_t* r_le, size_t r_stride_bytes,
                  size_t r_bytes, const uint8_t* rng_key32, uint64_t index_base, uint32_t* ct_out) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (N == 0) return 0;
  if (!ct || !ct_out) return fail(PAI_ERR_ARG, "pai_obfuscate: null buffer");
  if (obf_mode != PAI_OBF_GIVEN && obf_mode != PAI_OBF_RNG && obf_mode != PAI_OBF_POOL)
    return fail(PAI_ERR_ARG, "pai_obfuscate: obf_mode must be PAI_OBF_GIVEN, PAI_OBF_RNG or PAI_OBF_POOL");
  if (obf_mode == PAI_OBF_POOL) {   // the whole call or nothing: its chunks then take their entries in order
    const int prc = pool_check_take(c, N, "pai_obfuscate");
    if (prc) return prc;
  }
  if (obf_mode == PAI_OBF_GIVEN && (!r_le || r_bytes == 0 || r_bytes > (size_t)c->ct_words * 4))
    return fail(PAI_ERR_ARG, "pai_obfuscate: r must be given with 0 < r_bytes <= 4 ct_words");
  if (obf_mode == PAI_OBF_RNG && !rng_key32) return fail(PAI_ERR_ARG, "pai_obfuscate: rng key required");
  HIPCHK(hipSetDevice(c->device));
  const size_t W = c->ct_words;
  const size_t r_words = obf_mode == PAI_OBF_GIVEN ? (r_bytes + 3) / 4 : 0;
  const size_t r_cnt = obf_mode == PAI_OBF_GIVEN ? (r_stride_bytes ? N : 1) : 0;
  size_t CH;
  int nch, rc;
  if ((rc = host_pipe(c, N, carve_bytes({N * W * 4, r_cnt * r_words * 4}), W * 4, &CH, &nch))) return rc;
  Carve cv{(char*)c->d_hostio};
  uint32_t* dct = cv.take<uint32_t>(N * W);
  uint32_t* dr = cv.take<uint32_t>(r_cnt * r_words);
  hipStream_t sc = c->s_comp, sy = c->s_copy;
  if (r_cnt) {
    std::vector<uint32_t> hr(r_cnt * r_words, 0);
    for (size_t i = 0; i < r_cnt; ++i) std::memcpy(&hr[i * r_words], r_le + i * r_stride_bytes, r_bytes);
    HIPCHK(hipMemcpyAsync(dr, hr.data(), hr.size() * 4, hipMemcpyHostToDevice, sc));
    HIPCHK(hipStreamSynchronize(sc));   // hr is released at the end of this scope
  }
  const size_t r_stride_words = r_stride_bytes ? r_words : 0;
  ObfCall oc(c, obf_mode, (long long)N);   // one sampler decision for the call, whatever its chunks
  for (int i = 0; i < nch; ++i) {
    const size_t off = (size_t)i * CH, n = std::min(CH, N - off);
    if (i >= 2) HIPCHK(hipEventSynchronize(c->hev[i - 2]));   // the slot's previous upload is done
    par_copy(c->h_pin[i & 1], ct + off * W, n * W * 4);
    HIPCHK(hipMemcpyAsync(dct + off * W, c->h_pin[i & 1], n * W * 4, hipMemcpyHostToDevice, sy));
    HIPCHK(hipEventRecord(c->hev[i], sy));
    HIPCHK(hipStreamWaitEvent(sc, c->hev[i], 0));
    rc = pai_obfuscate_dev(c, dct + off * W, n, obf_mode, r_cnt ? dr + off * r_stride_words : nullptr, r_stride_words,
                           r_words, rng_key32, index_base + off, dct + off * W, sc);
    if (rc) {
      (void)hipStreamSynchronize(sc);
      (void)hipStreamSynchronize(sy);
      return rc;
    }
    HIPCHK(hipEventRecord(c->oev[i], sc));
  }
  HIPCHK(hipEventSynchronize(c->hev[nch - 1]));   // every upload has left the slots: they now carry the outputs
  auto d2h = [&](int i) -> int {
    const size_t off = (size_t)i * CH, n = std::min(CH, N - off);
    HIPCHK(hipStreamWaitEvent(sy, c->oev[i], 0));
    HIPCHK(hipMemcpyAsync(c->h_pin[i & 1], dct + off * W, n * W * 4, hipMemcpyDeviceToHost, sy));
    HIPCHK(hipEventRecord(c->pev[i], sy));
    return 0;
  };
  if ((rc = d2h(0))) return rc;
  for (int i = 0; i < nch; ++i) {
    if (i + 1 < nch && (rc = d2h(i + 1))) return rc;   // its slot's previous chunk (i - 1) is consumed
    const size_t off = (size_t)i * CH, n = std::min(CH, N - off);
    HIPCHK(hipEventSynchronize(c->pev[i]));
    par_copy(ct_out + off * W, c->h_pin[i & 1], n * W * 4);
  }
  HIPCHK(hipStreamSynchronize(sc));
  HIPCHK(hipStreamSynchronize(sy));
  return 0;
}

// The host-buffer sides of the pool: the words go up once into the host-io buffer and the device call follows on the
// context's compute stream; both wait for it, like their neighbours
static int pool_host_upload(pai_ctx* c, const std::vector<uint32_t>& words, uint32_t** d_out) {
  if (!c->s_comp) HIPCHK(hipStreamCreateWithFlags(&c->s_comp, hipStreamNonBlocking));
  if (c->tail_ev) HIPCHK(hipEventSynchronize(c->tail_ev));   // the buffer may still be read by the previous call
  const int rc = ensure_buf(&c->d_hostio, &c->hostio_bytes, std::max<size_t>(words.size(), 1) * 4);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(c->d_hostio, words.data(), words.size() * 4, hipMemcpyHostToDevice, c->s_comp));
  HIPCHK(hipStreamSynchronize(c->s_comp));
  *d_out = (uint32_t*)c->d_hostio;
  return 0;
}

int pai_pool_put(pai_ctx* c, const uint32_t* rho, size_t count) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (count == 0) return 0;
  if (!rho) return fail(PAI_ERR_ARG, "pai_pool_put: null buffer");
  int rc = pool_check_room(c, count, "pai_pool_put");
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  uint32_t* d = nullptr;
  if ((rc = pool_host_upload(c, std::vector<uint32_t>(rho, rho + count * c->ct_words), &d))) return rc;
  rc = pai_pool_put_dev(c, d, count, c->s_comp);
  HIPCHK(hipStreamSynchronize(c->s_comp));
  return rc;
}

int pai_pool_fill(pai_ctx* c, size_t count, int obf_mode, const uint8_t* r_le, size_t r_stride_bytes, size_t r_bytes,
                  const uint8_t* rng_key32, uint64_t index_base) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (obf_mode != PAI_OBF_GIVEN && obf_mode != PAI_OBF_RNG)
    return fail(PAI_ERR_ARG, "pai_pool_fill: obf_mode must be PAI_OBF_GIVEN or PAI_OBF_RNG");
  if (obf_mode == PAI_OBF_GIVEN && (!r_le || r_bytes == 0 || r_bytes > (size_t)c->ct_words * 4))
    return fail(PAI_ERR_ARG, "pai_pool_fill: r must be given with 0 < r_bytes <= 4 ct_words");
  if (obf_mode == PAI_OBF_RNG && !rng_key32) return fail(PAI_ERR_ARG, "pai_pool_fill: rng key required");
  if (count == 0) return 0;
  int rc = pool_check_room(c, count, "pai_pool_fill");
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  const size_t r_words = obf_mode == PAI_OBF_GIVEN ? (r_bytes + 3) / 4 : 0;
  const size_t r_cnt = obf_mode == PAI_OBF_GIVEN ? (r_stride_bytes ? count : 1) : 0;
  std::vector<uint32_t> hr(r_cnt * r_words, 0);
  for (size_t i = 0; i < r_cnt; ++i) std::memcpy(&hr[i * r_words], r_le + i * r_stride_bytes, r_bytes);
  uint32_t* dr = nullptr;
  if ((rc = pool_host_upload(c, hr, &dr))) return rc;
  rc = pai_pool_fill_dev(c, count, obf_mode, r_cnt ? dr : nullptr, r_stride_bytes ? r_words : 0, r_words, rng_key32,
                         index_base, c->s_comp);
  HIPCHK(hipStreamSynchronize(c->s_comp));
  return rc;
}

int pai_decrypt(pai_ctx* c, const uint32_t* ct, const int32_t* exp, size_t N, double* val_out, int64_t* mant_out,
                int32_t* status_out, uint32_t* raw_out) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (!c->has_priv) return fail(PAI_ERR_NOPRIV, "pai_decrypt: context has no private key");
  if (N == 0) return 0;
  if (!ct || !exp || !val_out || !status_out) return fail(PAI_ERR_ARG, "pai_decrypt: null buffer");
  HIPCHK(hipSetDevice(c->device));
  const size_t W = c->ct_words, P = raw_out ? c->pt_words : 0;
  size_t CH;
  int nch, rc;
  if ((rc = host_pipe(c, N, carve_bytes({N * W * 4, N * 4, N * 8, N * 8, N * 4, N * P * 4}), W * 4, &CH, &nch)))
    return rc;
  Carve cv{(char*)c->d_hostio};
  uint32_t* dct = cv.take<uint32_t>(N * W);
  int32_t* dexp = cv.take<int32_t>(N);
  double* dval = cv.take<double>(N);
  int64_t* dmant = cv.take<int64_t>(N);
  int32_t* dst = cv.take<int32_t>(N);
  uint32_t* draw = cv.take<uint32_t>(N * P);
  hipStream_t sc = c->s_comp, sy = c->s_copy;
  HostCall hc(c);
  for (int i = 0; i < nch; ++i) {
    const size_t off = (size_t)i * CH, n = std::min(CH, N - off);
    if (i >= 2) HIPCHK(hipEventSynchronize(c->hev[i - 2]));   // the slot's previous upload is done
    par_copy(c->h_pin[i & 1], ct + off * W, n * W * 4);
    HIPCHK(hipMemcpyAsync(dct + off * W, c->h_pin[i & 1], n * W * 4, hipMemcpyHostToDevice, sy));
    HIPCHK(hipMemcpyAsync(dexp + off, exp + off, n * 4, hipMemcpyHostToDevice, sy));
    HIPCHK(hipEventRecord(c->hev[i], sy));
    HIPCHK(hipStreamWaitEvent(sc, c->hev[i], 0));
    if ((rc = pai_decrypt_dev(c, dct + off * W, dexp + off, n, dval + off, dmant + off, dst + off,
                              raw_out ? draw + off * P : nullptr, sc))) {
      (void)hipStreamSynchronize(sc);
      return rc;
    }
  }
  HIPCHK(hipMemcpyAsync(val_out, dval, N * 8, hipMemcpyDeviceToHost, sc));
  if (mant_out) HIPCHK(hipMemcpyAsync(mant_out, dmant, N * 8, hipMemcpyDeviceToHost, sc));
  HIPCHK(hipMemcpyAsync(status_out, dst, N * 4, hipMemcpyDeviceToHost, sc));
  if (raw_out) HIPCHK(hipMemcpyAsync(raw_out, draw, N * P * 4, hipMemcpyDeviceToHost, sc));
  HIPCHK(hipStreamSynchronize(sc));
  return 0;
}

// Packed plaintexts on host buffers: the values go up once, the ciphertexts are cut into chunks like pai_encrypt's (a
// chunk of n ciphertexts takes the n slots values behind it) and drain through the pinned slots; one sampler decision
// for the call, counted in ciphertexts (ObfCall).
int pai_encrypt_packed(pai_ctx* c, int dtype, const void* x, size_t N, const pai_pack_layout* layout, int obf_mode,
                       const uint8_t* r_le, size_t r_stride_bytes, size_t r_bytes, const uint8_t* rng_key32,
                       uint64_t index_base, uint32_t* ct_out, int32_t* status_out) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  PackLayout lay;
  int rc = pack_layout(c, layout, &lay);
  if (rc) return rc;
  if (N == 0) return 0;
  if (dtype < 0 || dtype > 2 || !x || !ct_out) return fail(PAI_ERR_ARG, "pai_encrypt_packed: bad arguments");
  if (obf_mode < 0 || obf_mode > 2) return fail(PAI_ERR_ARG, "pai_encrypt_packed: bad obf_mode");
  if (obf_mode == PAI_OBF_GIVEN && (!r_le || r_bytes == 0 || r_bytes > (size_t)c->ct_words * 4))
    return fail(PAI_ERR_ARG, "pai_encrypt_packed: r must be given with 0 < r_bytes <= 4 ct_words");
  if (obf_mode == PAI_OBF_RNG && !rng_key32) return fail(PAI_ERR_ARG, "pai_encrypt_packed: rng key required");
  HIPCHK(hipSetDevice(c->device));
  const size_t esz = dtype == PAI_F32 ? 4 : 8, W = c->ct_words, K = lay.k, C = (N + K - 1) / K;
  const size_t r_words = obf_mode == PAI_OBF_GIVEN ? (r_bytes + 3) / 4 : 0;
  const size_t r_cnt = obf_mode == PAI_OBF_GIVEN ? (r_stride_bytes ? C : 1) : 0;
  size_t CH;
  int nch;
  if ((rc = host_pipe(c, C, carve_bytes({N * esz, C * W * 4, N * 4, r_cnt * r_words * 4}), W * 4, &CH, &nch))) return rc;
  Carve cv{(char*)c->d_hostio};
  void* dx = cv.take<uint8_t>(N * esz);
  uint32_t* dct = cv.take<uint32_t>(C * W);
  int32_t* dst = cv.take<int32_t>(N);
  uint32_t* dr = cv.take<uint32_t>(r_cnt * r_words);
  hipStream_t sc = c->s_comp, sy = c->s_copy;
  HIPCHK(hipMemcpyAsync(dx, x, N * esz, hipMemcpyHostToDevice, sc));
  if (r_cnt) {
    std::vector<uint32_t> hr(r_cnt * r_words, 0);
    for (size_t i = 0; i < r_cnt; ++i) std::memcpy(&hr[i * r_words], r_le + i * r_stride_bytes, r_bytes);
    HIPCHK(hipMemcpyAsync(dr, hr.data(), hr.size() * 4, hipMemcpyHostToDevice, sc));
    HIPCHK(hipStreamSynchronize(sc));   // hr is released at the end of this scope
  }
  const size_t r_stride_words = r_stride_bytes ? r_words : 0;
  ObfCall oc(c, obf_mode, (long long)C);
  for (int i = 0; i < nch; ++i) {
    const size_t off = (size_t)i * CH, n = std::min(CH, C - off), v0 = off * K, nv = std::min(n * K, N - v0);
    rc = pai_encrypt_packed_dev(c, dtype, (const char*)dx + v0 * esz, nv, layout, obf_mode,
                                r_cnt ? dr + off * r_stride_words : nullptr, r_stride_words, r_words, rng_key32,
                                index_base + off, dct + off * W, dst + v0, sc);
    if (rc) {
      (void)hipStreamSynchronize(sc);
      return rc;
    }
    HIPCHK(hipEventRecord(c->hev[i], sc));
  }
  auto d2h = [&](int i) -> int {
    const size_t off = (size_t)i * CH, n = std::min(CH, C - off);
    HIPCHK(hipStreamWaitEvent(sy, c->hev[i], 0));
    HIPCHK(hipMemcpyAsync(c->h_pin[i & 1], dct + off * W, n * W * 4, hipMemcpyDeviceToHost, sy));
    HIPCHK(hipEventRecord(c->pev[i], sy));
    return 0;
  };
  if ((rc = d2h(0))) return rc;
  for (int i = 0; i < nch; ++i) {
    if (i + 1 < nch && (rc = d2h(i + 1))) return rc;   // its slot's previous chunk (i - 1) is consumed
    const size_t off = (size_t)i * CH, n = std::min(CH, C - off);
    HIPCHK(hipEventSynchronize(c->pev[i]));
    par_copy(ct_out + off * W, c->h_pin[i & 1], n * W * 4);
  }
  if (status_out) HIPCHK(hipMemcpyAsync(status_out, dst, N * 4, hipMemcpyDeviceToHost, sc));
  HIPCHK(hipStreamSynchronize(sc));
  HIPCHK(hipStreamSynchronize(sy));
  return 0;
}

int pai_decrypt_packed(pai_ctx* c, const uint32_t* ct, const pai_pack_layout* layout, size_t N, double* val_out,
                       int64_t* mant_out, int32_t* status_out) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  PackLayout lay;
  int rc = pack_layout(c, layout, &lay);
  if (rc) return rc;
  if (!c->has_priv) return fail(PAI_ERR_NOPRIV, "pai_decrypt_packed: context has no private key");
  if (N == 0) return 0;
  if (!ct || !val_out || !status_out) return fail(PAI_ERR_ARG, "pai_decrypt_packed: null buffer");
  HIPCHK(hipSetDevice(c->device));
  const size_t W = c->ct_words, K = lay.k, C = (N + K - 1) / K;
  size_t CH;
  int nch;
  if ((rc = host_pipe(c, C, carve_bytes({C * W * 4, N * 8, N * 8, N * 4}), W * 4, &CH, &nch))) return rc;
  Carve cv{(char*)c->d_hostio};
  uint32_t* dct = cv.take<uint32_t>(C * W);
  double* dval = cv.take<double>(N);
  int64_t* dmant = cv.take<int64_t>(N);
  int32_t* dst = cv.take<int32_t>(N);
  hipStream_t sc = c->s_comp, sy = c->s_copy;
  HostCall hc(c);
  for (int i = 0; i < nch; ++i) {
    const size_t off = (size_t)i * CH, n = std::min(CH, C - off), v0 = off * K, nv = std::min(n * K, N - v0);
    if (i >= 2) HIPCHK(hipEventSynchronize(c->hev[i - 2]));   // the slot's previous upload is done
    par_copy(c->h_pin[i & 1], ct + off * W, n * W * 4);
    HIPCHK(hipMemcpyAsync(dct + off * W, c->h_pin[i & 1], n * W * 4, hipMemcpyHostToDevice, sy));
    HIPCHK(hipEventRecord(c->hev[i], sy));
    HIPCHK(hipStreamWaitEvent(sc, c->hev[i], 0));
    if ((rc = pai_decrypt_packed_dev(c, dct + off * W, layout, nv, dval + v0, dmant + v0, dst + v0, sc))) {
      (void)hipStreamSynchronize(sc);
      return rc;
    }
  }
  HIPCHK(hipMemcpyAsync(val_out, dval, N * 8, hipMemcpyDeviceToHost, sc));
  if (mant_out) HIPCHK(hipMemcpyAsync(mant_out, dmant, N * 8, hipMemcpyDeviceToHost, sc));
  HIPCHK(hipMemcpyAsync(status_out, dst, N * 4, hipMemcpyDeviceToHost, sc));
  HIPCHK(hipStreamSynchronize(sc));
  return 0;
}

// Chunks of whole outputs (multiples of `slots` values, like pai_encrypt_packed): the inputs of chunk i + 1 go up through
// the pinned slots while chunk i folds; the outputs, `slots` times smaller, come down at the end.
int pai_pack_ciphertexts(pai_ctx* c, const uint32_t* ct, const int32_t* exp, size_t N, const pai_pack_layout* layout,
                         uint32_t* ct_out, int32_t* status_out) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  PackLayout lay;
  int rc = pack_layout(c, layout, &lay);
  if (rc) return rc;
  if (N == 0) return 0;
  if (!ct || !exp || !ct_out) return fail(PAI_ERR_ARG, "pai_pack_ciphertexts: null buffer");
  HIPCHK(hipSetDevice(c->device));
  const size_t W = c->ct_words, K = lay.k, C = (N + K - 1) / K;
  size_t CH;
  int nch;
  if ((rc = host_pipe(c, C, carve_bytes({N * W * 4, N * 4, C * W * 4, N * 4}), K * W * 4, &CH, &nch))) return rc;
  Carve cv{(char*)c->d_hostio};
  uint32_t* dct = cv.take<uint32_t>(N * W);
  int32_t* dexp = cv.take<int32_t>(N);
  uint32_t* dout = cv.take<uint32_t>(C * W);
  int32_t* dst = cv.take<int32_t>(N);
  hipStream_t sc = c->s_comp, sy = c->s_copy;
  HostCall hc(c);
  FoldCall fc(c, C);
  HIPCHK(hipMemcpyAsync(dexp, exp, N * 4, hipMemcpyHostToDevice, sc));
  for (int i = 0; i < nch; ++i) {
    const size_t off = (size_t)i * CH, n = std::min(CH, C - off), v0 = off * K, nv = std::min(n * K, N - v0);
    if (i >= 2) HIPCHK(hipEventSynchronize(c->hev[i - 2]));   // the slot's previous upload is done
    par_copy(c->h_pin[i & 1], ct + v0 * W, nv * W * 4);
    HIPCHK(hipMemcpyAsync(dct + v0 * W, c->h_pin[i & 1], nv * W * 4, hipMemcpyHostToDevice, sy));
    HIPCHK(hipEventRecord(c->hev[i], sy));
    HIPCHK(hipStreamWaitEvent(sc, c->hev[i], 0));
    if ((rc = pai_pack_ciphertexts_dev(c, dct + v0 * W, dexp + v0, nv, layout, dout + off * W, dst + v0, sc))) {
      (void)hipStreamSynchronize(sc);
      return rc;
    }
  }
  HIPCHK(hipMemcpyAsync(ct_out, dout, C * W * 4, hipMemcpyDeviceToHost, sc));
  if (status_out) HIPCHK(hipMemcpyAsync(status_out, dst, N * 4, hipMemcpyDeviceToHost, sc));
  HIPCHK(hipStreamSynchronize(sc));
  return 0;
}

// Chunks of whole outputs (multiples of `group` inputs), as pai_pack_ciphertexts: the inputs of chunk i + 1 go up through
// the pinned slots while chunk i folds; the outputs come down at the end.
int pai_repack(pai_ctx* c, const uint32_t* ct, size_t N, const pai_pack_layout* in_layout, int group, uint32_t* ct_out) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  PackLayout lay;
  int rc = pack_layout(c, in_layout, &lay);
  if (rc) return rc;
  if (group < 1 || (long long)lay.k * group > (c->nb - 2) / lay.sb)
    return fail(PAI_ERR_ARG, "pai_repack: slots * group must be in [slots, (key_bits - 2) / slot_bits]");
  if (N == 0) return 0;
  if (!ct || !ct_out) return fail(PAI_ERR_ARG, "pai_repack: null buffer");
  const size_t W = c->ct_words, K = (size_t)group, C = (N + K - 1) / K;
  if (ranges_overlap(ct, N * W * 4, ct_out, C * W * 4)) return fail(PAI_ERR_ARG, "pai_repack: ct_out must not overlap ct");
  HIPCHK(hipSetDevice(c->device));
  size_t CH;
  int nch;
  if ((rc = host_pipe(c, C, carve_bytes({N * W * 4, C * W * 4}), K * W * 4, &CH, &nch))) return rc;
  Carve cv{(char*)c->d_hostio};
  uint32_t* dct = cv.take<uint32_t>(N * W);
  uint32_t* dout = cv.take<uint32_t>(C * W);
  hipStream_t sc = c->s_comp, sy = c->s_copy;
  HostCall hc(c);
  FoldCall fc(c, C);
  for (int i = 0; i < nch; ++i) {
    const size_t off = (size_t)i * CH, n = std::min(CH, C - off), v0 = off * K, nv = std::min(n * K, N - v0);
    if (i >= 2) HIPCHK(hipEventSynchronize(c->hev[i - 2]));   // the slot's previous upload is done
    par_copy(c->h_pin[i & 1], ct + v0 * W, nv * W * 4);
    HIPCHK(hipMemcpyAsync(dct + v0 * W, c->h_pin[i & 1], nv * W * 4, hipMemcpyHostToDevice, sy));
    HIPCHK(hipEventRecord(c->hev[i], sy));
    HIPCHK(hipStreamWaitEvent(sc, c->hev[i], 0));
    if ((rc = pai_repack_dev(c, dct + v0 * W, nv, in_layout, group, dout + off * W, sc))) {
      (void)hipStreamSynchronize(sc);
      return rc;
    }
  }
  HIPCHK(hipMemcpyAsync(ct_out, dout, C * W * 4, hipMemcpyDeviceToHost, sc));
  HIPCHK(hipStreamSynchronize(sc));
  return 0;
}

// ------------------------------------------------------------------ device-resident buffers (engine_res.hip)
namespace fpai {
hipError_t shared_dev_malloc(void** p, size_t bytes) { return dev_malloc(p, bytes); }
void shared_par_copy(void* dst, const void* src, size_t bytes) { par_copy(dst, src, bytes); }
}  // namespace fpai

// Gather of rows by a host index (kernels_res.hpp k_take). Every argument is checked before the first launch, so no
// index formed from data addresses outside the input.
int pai_take_dev(pai_ctx* c, const uint32_t* d_ct, const int32_t* d_exp, size_t N, const int64_t* index, size_t M,
                 uint32_t* d_ct_out, int32_t* d_exp_out, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  if (M == 0) return 0;
  if (!index || !d_ct_out || !d_exp_out || (N > 0 && (!d_ct || !d_exp)))
    return fail(PAI_ERR_ARG, "pai_take_dev: null pointer");
  if (N >= ((size_t)1 << 40) || M >= ((size_t)1 << 40)) return fail(PAI_ERR_ARG, "pai_take_dev: too many rows");
  for (size_t j = 0; j < M; ++j)
    if (index[j] < -1 || index[j] >= (int64_t)N) return fail(PAI_ERR_ARG, "pai_take_dev: index out of range");
  const size_t W = c->ct_words;
  if (ranges_overlap(d_ct, N * W * 4, d_ct_out, M * W * 4) || ranges_overlap(d_exp, N * 4, d_exp_out, M * 4) ||
      ranges_overlap(d_ct, N * W * 4, d_exp_out, M * 4) || ranges_overlap(d_exp, N * 4, d_ct_out, M * W * 4) ||
      ranges_overlap(d_ct_out, M * W * 4, d_exp_out, M * 4))
    return fail(PAI_ERR_ARG, "pai_take_dev: the output overlaps the input");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  int rc = ensure_buf(&c->d_take, &c->take_bytes, std::max<size_t>(M * 8, 16));
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(c->d_take, index, M * 8, hipMemcpyHostToDevice, st));
  TakeParams p{d_ct, d_exp, (const long long*)c->d_take, (long long)M, (int)W, d_ct_out, d_exp_out};
  HIPCHK(take_launch(p, c->cus, st));
  HIPCHK(hipStreamSynchronize(st));   // the index is the caller's host memory, and d_take serves the next call
  return 0;
}

// ------------------------------------------------------------------ index lists on the device
// The index (and the segment offsets) are device memory, so nothing here can look at them: k_check_idx runs first on
// the stream and leaves the smallest offenders in d_bad, and every kernel behind it reads those two words before it
// touches anything (TakeParams.gate, AddParams.gate, SegPlanParams.gate, SegRowsParams.gate). No wait on the host, no
// copy to the host, scratch from the context.
static int check_idx(pai_ctx* c, const int64_t* d_index, size_t total, long long lo, size_t N, const int64_t* d_seg_off,
                     size_t nseg, int64_t* d_bad, hipStream_t st) {
  HIPCHK(hipMemsetAsync(d_bad, 0xFF, 16, st));
  CheckIdxParams p{(const long long*)d_index, (long long)total, lo, (long long)N, (const long long*)d_seg_off,
                   (long long)nseg, (unsigned long long*)d_bad};
  HIPCHK(check_idx_launch(p, c->cus, st));
  return 0;
}

int pai_take_idx_dev(pai_ctx* c, const uint32_t* d_ct, const int32_t* d_exp, size_t N, const int64_t* d_index, size_t M,
                     int allow_empty, uint32_t* d_ct_out, int32_t* d_exp_out, int64_t* d_bad, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  if (!d_bad) return fail(PAI_ERR_ARG, "pai_take_idx_dev: null pointer");
  if (M > 0 && (!d_index || !d_ct_out || !d_exp_out || (N > 0 && (!d_ct || !d_exp))))
    return fail(PAI_ERR_ARG, "pai_take_idx_dev: null pointer");
  if (N >= ((size_t)1 << 40) || M >= ((size_t)1 << 40)) return fail(PAI_ERR_ARG, "pai_take_idx_dev: too many rows");
  const size_t W = c->ct_words;
  const struct { const void* p; size_t n; } in[] = {{d_ct, N * W * 4}, {d_exp, N * 4}, {d_index, M * 8}, {d_bad, 16}},
                                            out[] = {{d_ct_out, M * W * 4}, {d_exp_out, M * 4}};
  for (const auto& o : out)
    for (const auto& i : in)
      if (i.n && o.n && ranges_overlap(i.p, i.n, o.p, o.n))
        return fail(PAI_ERR_ARG, "pai_take_idx_dev: the output overlaps the input");
  if (M && (ranges_overlap(d_ct_out, M * W * 4, d_exp_out, M * 4) || ranges_overlap(d_bad, 16, d_index, M * 8)))
    return fail(PAI_ERR_ARG, "pai_take_idx_dev: the output overlaps the input");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  int rc = check_idx(c, d_index, M, allow_empty ? -1 : 0, N, nullptr, 0, d_bad, st);
  if (rc || M == 0) return rc;
  TakeParams p{d_ct, d_exp, (const long long*)d_index, (long long)M, (int)W, d_ct_out, d_exp_out, (const long long*)d_bad};
  HIPCHK(take_launch(p, c->cus, st));
  return 0;
}

// The tree of pai_segment_add_dev (parts of SEG_CHUNK members through k_add with gather rows), planned on the device.
// The host knows `total` and `nseg` only, so it launches LEVELS = the smallest l >= 1 with 16^l >= total levels: no
// segment is longer than total, so after l - 1 levels every segment is down to at most 16 rows and the last level writes
// one row per segment. A segment that is finished earlier passes through: a part of one member is that member again
// (k_add of one operand below n^2 multiplies nothing), so the bits are those of the host-list call. Level k launches
// k_add over total / 16^(k + 1) + nseg rows, the host's bound on its parts; the rows past the real count gather nothing
// and write the identity into scratch that nobody reads.
int pai_segment_add_idx_dev(pai_ctx* c, const uint32_t* d_ct, const int32_t* d_exp, size_t N, const int64_t* d_index,
                            size_t total, const int64_t* d_seg_off, size_t nseg, uint32_t* d_out, int32_t* d_exp_out,
                            int64_t* d_bad, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  if (!d_bad || !d_seg_off) return fail(PAI_ERR_ARG, "pai_segment_add_idx_dev: null pointer");
  if ((nseg > 0 && (!d_out || !d_exp_out)) || (total > 0 && (!d_index || !d_ct || !d_exp)))
    return fail(PAI_ERR_ARG, "pai_segment_add_idx_dev: null pointer");
  // k_add numbers its instances with an int (the schedule sort's perm)
  if (N >= ((size_t)1 << 40) || total >= ((size_t)1 << 40) || nseg >= ((size_t)1 << 30) ||
      total / SEG_CHUNK + nseg >= ((size_t)1 << 31))
    return fail(PAI_ERR_ARG, "pai_segment_add_idx_dev: too many rows");
  const size_t W = c->ct_words;
  const struct { const void* p; size_t n; } in[] = {{d_ct, N * W * 4}, {d_exp, N * 4}, {d_index, total * 8},
                                                    {d_seg_off, (nseg + 1) * 8}, {d_bad, 16}},
                                            out[] = {{d_out, nseg * W * 4}, {d_exp_out, nseg * 4}};
  for (const auto& o : out)
    for (const auto& i : in)
      if (i.n && o.n && ranges_overlap(i.p, i.n, o.p, o.n))
        return fail(PAI_ERR_ARG, "pai_segment_add_idx_dev: the output overlaps the input");
  if ((nseg && ranges_overlap(d_out, nseg * W * 4, d_exp_out, nseg * 4)) ||
      (total && ranges_overlap(d_bad, 16, d_index, total * 8)) || ranges_overlap(d_bad, 16, d_seg_off, (nseg + 1) * 8))
    return fail(PAI_ERR_ARG, "pai_segment_add_idx_dev: the output overlaps the input");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  int rc = check_idx(c, d_index, total, 0, N, d_seg_off, nseg, d_bad, st);
  if (rc || nseg == 0) return rc;
  const int C = SEG_CHUNK;
  static_assert(SEG_CHUNK == SEGPLAN_C, "the plan kernels cut segments as the host-list call does");
  int levels = 1;
  for (size_t cap = C; cap < total; cap *= C) ++levels;
  const size_t P = total / C + nseg;   // no level has more partial sums
  const size_t o_a = 0, o_b = align16(o_a + P * W * 4), o_ea = align16(o_b + P * W * 4), o_eb = align16(o_ea + P * 4),
               o_off = align16(o_eb + P * 4), o_g = align16(o_off + (size_t)(levels - 1) * (nseg + 1) * 8),
               need = align16(o_g + std::max(P, nseg) * C * 8);
  if ((rc = ensure_buf(&c->d_seg, &c->seg_bytes, need))) return rc;
  char* b = (char*)c->d_seg;
  uint32_t* part[2] = {(uint32_t*)(b + o_a), (uint32_t*)(b + o_b)};
  int32_t* pexp[2] = {(int32_t*)(b + o_ea), (int32_t*)(b + o_eb)};
  long long* d_off = (long long*)(b + o_off);
  long long* d_g = (long long*)(b + o_g);
  const long long* gate = (const long long*)d_bad;
  if (levels > 1) {
    SegPlanParams sp{(const long long*)d_seg_off, (long long)nseg, levels, d_off, gate};
    HIPCHK(seg_offsets_launch(sp, st));
  }
  const uint32_t* in_ct = d_ct;
  const int32_t* in_e = d_exp;
  size_t cap = total;   // bound on the rows that enter level k, without the nseg term
  for (int k = 0; k < levels; ++k) {
    const bool last = k == levels - 1;
    cap /= C;
    const long long rows = last ? (long long)nseg : (long long)(cap + nseg);
    SegRowsParams rp{};
    rp.in_off = k == 0 ? (const long long*)d_seg_off : d_off + (size_t)(k - 1) * (nseg + 1);
    rp.index = k == 0 ? (const long long*)d_index : nullptr;
    rp.out_off = last ? nullptr : d_off + (size_t)k * (nseg + 1);
    rp.nseg = (long long)nseg;
    rp.rows = rows;
    rp.gidx = d_g;
    rp.gate = gate;
    HIPCHK(seg_rows_launch(rp, c->cus, st));
    uint32_t* o = last ? d_out : part[k & 1];
    int32_t* oe = last ? d_exp_out : pexp[k & 1];
    AddParams ap = add_params(in_ct, in_e, C, rows, o, oe, d_g);
    ap.gate = gate;
    if ((rc = run_add(c, ap, st))) return rc;
    in_ct = o;
    in_e = oe;
  }
  return 0;
}

// The wire-ingest range check on the device (k_check_below): one read-back of one word.
int pai_check_below_dev(pai_ctx* c, const uint32_t* d_ct, size_t N, int64_t* first_bad, void* stream) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c, (hipStream_t)stream);
  if (!first_bad) return fail(PAI_ERR_ARG, "pai_check_below_dev: null pointer");
  *first_bad = -1;
  if (N == 0) return 0;
  if (!d_ct) return fail(PAI_ERR_ARG, "pai_check_below_dev: null pointer");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (!c->d_nsq32 && (rc = upload(c, c->N.words(c->ct_words), &c->d_nsq32))) return rc;
  if ((rc = ensure_buf(&c->d_take, &c->take_bytes, 16))) return rc;
  unsigned long long* d_first = (unsigned long long*)c->d_take;
  HIPCHK(hipMemsetAsync(d_first, 0xFF, 8, st));
  CheckBelowParams p{d_ct, (long long)N, c->ct_words, c->d_nsq32, d_first};
  HIPCHK(check_below_launch(p, c->cus, st));
  unsigned long long first = 0;
  HIPCHK(hipMemcpyAsync(&first, d_first, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (first != ~0ull) *first_bad = (int64_t)first;
  return 0;
}

// ------------------------------------------------------------------ debugging hooks (tests / tools only)
// The encrypt route of a context with these facts (encrypt_route.hpp); needs no context and no device.
int pai_debug_encrypt_route(const pai_route_facts* facts, int obf_mode, long long n, int r_words, int* sampler,
                            int* chain) {
  if (!facts || obf_mode < 0 || obf_mode > 2) return fail(PAI_ERR_ARG, "pai_debug_encrypt_route: bad arguments");
  const EncryptRoute rt = encrypt_route(*facts, obf_mode, n, r_words);
  if (sampler) *sampler = rt.sampler;
  if (chain) *chain = rt.chain;
  return 0;
}

// Copies the per-half sampler outputs (c0 G_h^a_h mod h^2) of the last fixed-base chunk: limbs [2][SB][n] (4096-bit
// keys), or canonical pairs [2][2S][n] with *sb = 2S for the pair tables (k_fbs/k_fbp; the p half times q^-2).
extern "C" int pai_debug_fb_w(pai_ctx* c, uint32_t* out, size_t max_words, long long* n, int* sb) {
  if (!c) return fail(PAI_ERR_ARG, "null ctx");
  CtxLock lk(c);
  if (!c->fb_last_w) return fail(PAI_ERR_ARG, "no fixed-base output");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());
  const int rows = c->fb.pair_s ? 2 * c->fb.pair_s : c->crt_sb;
  const long long ne = c->fb_last_n;
  const size_t words = (size_t)2 * rows * ne;
  if (words > max_words) return fail(PAI_ERR_ARG, "buffer too small");
  if (c->fb.pair_s) {   // 64-element tiles (kernels_fbp.hpp fbp_pair_index) -> [2][2S][n]
    const long long np = fbp_npad(ne);
    std::vector<uint32_t> t((size_t)2 * rows * np);
    HIPCHK(hipMemcpy(t.data(), c->fb_last_w, t.size() * 4, hipMemcpyDeviceToHost));
    for (int h = 0; h < 2; ++h)
      for (int j = 0; j < rows; ++j)
        for (long long i = 0; i < ne; ++i)
          out[((size_t)h * rows + j) * ne + i] = t[(size_t)h * rows * np + (size_t)(i >> 6) * rows * 64 + (size_t)j * 64 + (i & 63)];
  } else {
    HIPCHK(hipMemcpy(out, c->fb_last_w, words * 4, hipMemcpyDeviceToHost));
  }
  *n = c->fb_last_n;
  *sb = rows;
  return 0;
}

// ------------------------------------------------------------------ engine unit-test hook (test build only)
#if FLEXPAI_XCHECK
template <int TPI>
static int launch_debug(pai_ctx* c, DbgParams& p) {
  constexpr int S = TPI * L;
  constexpr int GPB = BLOCK / TPI;
  const size_t lds = (size_t)GPB * S * 4;
  const int grid = (int)((p.n + GPB - 1) / GPB);
  int rc = ensure_scratch(c, (size_t)grid * BLOCK * TILE_WORDS_PER_LANE * 4);
  if (rc) return rc;
  p.scratch = (uint32_t*)c->d_scratch;
  hipLaunchKernelGGL(k_debug<TPI>, dim3(grid), dim3(BLOCK), lds, (hipStream_t)0, p);
  HIPCHK(hipGetLastError());
  return 0;
}

#endif

extern "C" int pai_debug_engine(pai_ctx* c, int op, const uint32_t* a, const uint32_t* b, size_t N, uint32_t* out,
                                int32_t* flag) {
#if !FLEXPAI_XCHECK
  (void)c, (void)op, (void)a, (void)b, (void)N, (void)out, (void)flag;
  return fail(PAI_ERR_ARG, "pai_debug_engine: in the test build (libflexpai_xcheck.so) only");
#else
  if (!c || N == 0) return fail(PAI_ERR_ARG, "pai_debug_engine: bad args");
  CtxLock lk(c);
  HIPCHK(hipSetDevice(c->device));
  DevScope ds;
  const size_t W = c->ct_words;
  uint32_t* da = ds.alloc<uint32_t>(N * W);
  uint32_t* db = ds.alloc<uint32_t>(N * W);
  uint32_t* dout = ds.alloc<uint32_t>(N * W);
  int32_t* dflag = ds.alloc<int32_t>(N);
  HIPCHK(hipMemcpy(da, a, N * W * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(db, b, N * W * 4, hipMemcpyHostToDevice));
  DbgParams p{op, da, db, dout, dflag, (long long)N, (int)W, c->d_N, c->d_R2, c->d_nl, c->mprime_N,
              c->d_prog, c->nprog, nullptr};
  int rc = 0;
  switch (c->tpi_e) {
    case 2: rc = launch_debug<2>(c, p); break;
    case 4: rc = launch_debug<4>(c, p); break;
    case 8: rc = launch_debug<8>(c, p); break;
  }
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, dout, N * W * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(flag, dflag, N * 4, hipMemcpyDeviceToHost));
  return 0;
#endif
}
