// Which kernels an encrypt call runs on: the one place that decides it. A pure function of the context's facts
// (pai_route_facts, flexpai.h) and the call's obfuscator mode, element count and r width; it knows neither HIP nor
// pai_ctx, so pai_debug_encrypt_route can hand it to a test without a device.
//
// For an explicit r every chain gives the same ciphertext bits, so a wrong route shows only as a slower kernel (or as
// other bits under device RNG): tests/test_route_cpu.py pins the table.
#pragma once
#include "flexpai.h"

namespace fpai {

struct EncryptRoute {
  int sampler;   // PAI_SAMPLER_*: the fixed-base tables the call is eligible for
  int chain;     // PAI_CHAIN_*: the per-element kernels it runs on when those tables are not wanted or cannot be built
};

// r_words: the words of r the kernels will read (the caller's r_words for PAI_OBF_GIVEN, the context's stream words for
// PAI_OBF_RNG). The caller counts the call towards a sampler's break-even and builds its tables only for the sampler
// named here. The order, first match wins:
//   PAI_OBF_NONE                                      k_encrypt
//   key holder, CRT on, device RNG, fixed base on     key holder's sampler, ahead of the rows (resident or wanted
//                                                     tables take precedence over them)
//   4096-bit key holder, n <= crtw_max, r fits        k_crt_w<74, 148>; an r too wide for the rows goes on down
//   1024/2048-bit key holder                          k_crt_w at n <= crtw_max, lane CRT above (both reject an
//                                                     over-wide r with PAI_ERR_ARG, in launch_crt)
//   4096-bit key holder, n > crt4_min                 k_crt4_*
//   device RNG, public fixed base on, 2048-bit n      public sampler, ahead of k_pe_w
//   n <= crtw_max and a k_pe_w op list                k_pe_w
//   2048 / 1024 / 4096 bits                           k_pe_* / k_pe1_* / k_pe4_* (the last without a private key only)
//   otherwise                                         k_encrypt
inline EncryptRoute encrypt_route(const pai_route_facts& f, int obf_mode, long long n, int r_words) {
  EncryptRoute rt{PAI_SAMPLER_NONE, PAI_CHAIN_ENCRYPT};
  if (obf_mode == PAI_OBF_NONE) return rt;
  const bool rng = obf_mode == PAI_OBF_RNG, crt = f.crt_enabled != 0;
  const bool lane = f.crt_ok && crt && (f.crt_sa == 19 || f.crt_sa == 37);
  if (rng && f.fbg_ok && crt && f.fb_enabled) rt.sampler = PAI_SAMPLER_KEY;
  if (f.rows_sa && crt && n <= f.crtw_max && r_words <= f.rows_r_max) {
    rt.chain = PAI_CHAIN_CRT_ROWS4;
  } else if (lane) {
    if (rng && f.fb_enabled) rt.sampler = PAI_SAMPLER_KEY;
    rt.chain = n <= f.crtw_max ? PAI_CHAIN_CRT_ROWS : PAI_CHAIN_CRT_LANE;
  } else if (f.crt4_ok && crt && n > f.crt4_min) {
    rt.chain = PAI_CHAIN_CRT4;
  } else {
    if (rng && f.pfb_enabled && f.pfb_supported && rt.sampler == PAI_SAMPLER_NONE) rt.sampler = PAI_SAMPLER_PUBLIC;
    if (n <= f.crtw_max && f.pew_ok) rt.chain = PAI_CHAIN_PE_ROWS;
    else if (f.pe_ok && f.ct_words == 128) rt.chain = PAI_CHAIN_PE;   // 2033..2048-bit n: k_pe_fin writes 64-word pairs
    else if (f.pe1_ok) rt.chain = PAI_CHAIN_PE1;
    else if (f.pe4_ok && !f.has_priv) rt.chain = PAI_CHAIN_PE4;
  }
  return rt;
}

}  // namespace fpai
