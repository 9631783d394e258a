/*
 * flexpai — MI355X-native Paillier array engine, C ABI.
 *
 * Drop-in boundary for tongdun/iBond-flex `flex.crypto.paillier` (Python). Each entry point
 * replaces the per-element gmpy2 work that the reference does on the CPU:
 *
 *   pai_ctx_create        <- PaillierPublicKey(n)                  flex/crypto/paillier/keypair.py:20-39
 *   pai_ctx_set_private   <- PaillierPrivateKey(pk, p, q)          flex/crypto/paillier/keypair.py:42-90
 *   pai_ctx_set_option    <- (no reference counterpart: selects the CRT encryption kernels)
 *   pai_encrypt[_dev]     <- PaillierEncryptor.encrypt(ndarray)    flex/crypto/paillier/encryptor.py:71-114
 *                            (FixedPointNumber.encode fixedpoint_number.py:46-90, raw_encrypt
 *                             raw_encrypt.py:22-49, apply_obfuscation obfuscator.py:23-37 ->
 *                             gmpy_math.powmod/mulmod gmpy_math.py:43-63)
 *   pai_add[_dev]         <- sum of PaillierEncryptedNumber arrays encrypted_number.py:65-69,
 *                            115-137, 166-185 (k-way, order independent)
 *   pai_decrypt[_dev]     <- PaillierDecryptor.decrypt(ndarray)    flex/crypto/paillier/decryptor.py:33-127
 *                            (+ FixedPointNumber.decode fixedpoint_number.py:92-107)
 *   pai_mul[_dev]         <- PaillierEncryptedNumber.__mul__ / __rmul__ over arrays (encrypted_number.py:80-113;
 *                            parallel_ops.mul parallel_ops.py:23-44): c^s, or invert(c)^(n-s) for negatives
 *   pai_add_plain[_dev]   <- PaillierEncryptedNumber + plain scalar over arrays (encrypted_number.py:65-72,
 *                            139-164 __add_scalar/__add_fixpointnumber; parallel_ops.add parallel_ops.py:47-72)
 *   pai_segment_add[_dev] <- per-bin sums sum(y[i]) over index lists (hetero_bin.py:28-36, IV_FFS
 *                            iv_ffs/compute.py:77-93): one k-way aligned product per segment
 *   pai_matmul[_dev]      <- ndarray.dot of encrypted by plain (he_otp_lr_ft1/train.py:160,
 *                            he_otp_lr_ft2/train.py:188): per output sum_k c_ik (x) x_kj, i.e. __mul__ then
 *                            __add__ (encrypted_number.py:65-69, 86-113, 166-185)
 *   pai_segment_dot[_dev] <- the same dot over the STORED entries of a sparse plain matrix, and weighted per-bin
 *                            sums: per segment sum_t c[index[t]] (x) x[t], __mul__ then __add__
 *   pai_obfuscate[_dev]   <- PaillierEncryptedNumber.apply_obfuscation / ciphertext(be_secure=True) over arrays
 *                            (encrypted_number.py:50-63 -> apply_obfuscation obfuscator.py:23-37): c * r^n mod n^2
 *   pai_pool_*            <- (no reference counterpart) r^n mod n^2 drawn ahead of time into a ring of the context; PAI_OBF_POOL
 *                            encryptions and re-randomisations then spend one entry each, (1 + n m) rho mod n^2
 *   pai_next_prime        <- gmpy2.next_prime(r) of getprimeover    flex/crypto/gmpy_math.py:77-87, the two prime
 *                            searches of generate_paillier_keypair  flex/crypto/paillier/keypair.py:93-127 (one batch):
 *                            a sieve by the odd primes below 2000 on the host, then Miller-Rabin on 16-lane rows
 *                            (kernels_prime.hpp k_mr_w: base 3 over every survivor of a window, the other 39 bases
 *                            over the smallest one left). Same primes as the package's host search
 *                            (_bigint.next_prime), which reproduces the reference's seeded keys
 *   pai_prime_test        <- (no reference counterpart) the strong-probable-prime verdicts of that kernel for
 *                            given candidates and bases; pai_debug_prime_sieve: the sieve alone, on the host
 *   pai_comm_* / pai_allgather_*  <- (no reference counterpart: the reference encrypts on one host's CPU
 *                            pool, encryptor.py:71-97) reassembly of ciphertext shards encrypted on
 *                            several GPUs, one RCCL all-gather over xGMI
 *
 * Conventions
 *   - Integers cross the boundary as little-endian bytes (key material) or little-endian 32-bit
 *     words, one ciphertext contiguous (AoS): ciphertext i occupies words [i*W, (i+1)*W) with
 *     W = pai_ct_words(ctx) = 2*key_bits/32. This is zero-copy with Python int.to_bytes(...,'little').
 *   - Host-buffer entry points are synchronous and never retain caller memory.
 *   - *_dev entry points take device pointers and a hipStream_t (as void*) and are asynchronous.
 *   - Return value 0 = success; negative = error, message in pai_last_error() (thread local).
 *   - Per-element outcomes are reported in an int32 status array (PAI_EL_*), mapped by the Python
 *     layer onto the reference's exceptions.
 *   - Threads: a context may be shared by several threads. Every entry point that takes a pai_ctx holds
 *     the context's (recursive) mutex for the whole call, and a *_dev call's stream first waits for the
 *     device work of the context's previous call, whatever stream that was on (the context's scratch,
 *     work and table buffers are shared by all its calls). Calls on one context therefore run one after
 *     the other; contexts of different keys run concurrently. pai_ctx_destroy must not race other calls
 *     on the same context. (The reference never shares this state: it pickles the key into pool
 *     processes, encryptor.py:89-96.)
 *   - Reproducibility: PAI_OBF_RNG ciphertexts depend only on (rng_key, global index) for a given sampler,
 *     but the sampler is chosen per context: the fixed-base tables are built only once a context has seen
 *     the break-even element count (pai_ctx_fixed_base_policy). Two process layouts (one process vs
 *     sharded ranks, whose shards may sit below the threshold) give the same bits only when the tables are
 *     built up front (pai_ctx_fixed_base_prepare / pai_ctx_public_fb_prepare) or $FLEXPAI_FB_MIN_ELEMS /
 *     $FLEXPAI_PFB_MIN_ELEMS = 0; otherwise the outputs differ in bits but decrypt identically and have
 *     the same distribution.
 */
#ifndef FLEXPAI_H
#define FLEXPAI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pai_ctx pai_ctx;
typedef struct pai_comm pai_comm;

/* return codes */
#define PAI_OK 0
#define PAI_ERR_ARG (-1)
#define PAI_ERR_HIP (-2)
#define PAI_ERR_NOPRIV (-3)
#define PAI_ERR_KEY (-4)
#define PAI_ERR_NOINV (-5)  /* a ciphertext has no inverse mod n^2 (gmpy_math.invert ZeroDivisionError) */

/* input dtypes for pai_encrypt */
#define PAI_F32 0
#define PAI_F64 1
#define PAI_I64 2

/* obfuscation modes (SURVEY.md §8b randomness contract) */
#define PAI_OBF_NONE 0   /* random_value == 0 : c = 1 + n*m                      (encryptor.py:61-67) */
#define PAI_OBF_GIVEN 1  /* explicit r per element (r_stride 0 = one r for all)  (obfuscator.py:35)  */
#define PAI_OBF_RNG 2    /* device ChaCha20 CSPRNG keyed by rng_key, nonce = global element index    */
#define PAI_OBF_POOL 3   /* take the call's obfuscators from the context's pool, in order, each exactly once
                            (pai_pool_*, below); pai_encrypt[_dev] and pai_obfuscate[_dev] only              */

/* exponent modes for encode (fixedpoint_number.py:63-82) */
#define PAI_EXP_AUTO 0   /* precision=None: exponent from frexp / 0 for ints */
#define PAI_EXP_FIXED 1  /* precision given: exponent = fixed_exp for every element */

/* per-element status */
#define PAI_EL_OK 0           /* float result in val_out                                            */
#define PAI_EL_INT 1          /* exponent <= 0: exact integer mant_out * 16^(-exp) (fits int64)      */
#define PAI_EL_INT_BIG 2      /* exponent <= 0 and the mantissa does not fit int64 (use raw_out)     */
#define PAI_EL_OVERFLOW 3     /* OverflowError('Overflow detected in decode number')  :104-105     */
#define PAI_EL_FLOAT_OVF 4    /* OverflowError: int too large to convert to float (e > 0)           */
#define PAI_EL_ENC_RANGE 5    /* encode ValueError (fixedpoint_number.py:86-88) / beyond int64      */

/* context options */
#define PAI_OPT_CRT_ENCRYPT 1    /* 1 (default): encrypt via the private-key CRT path when available */
#define PAI_OPT_CRT_AVAILABLE 2  /* read-only: 1 when the private key is set and the CRT kernels fit */
#define PAI_OPT_STAGE_TIMING 3   /* 1: record HIP events between the kernels of each encrypt/decrypt call */
#define PAI_OPT_LANE_DECRYPT 4   /* 1 (default): decrypt on the lane engine when the key halves fit it;
                                    0: lane-group kernel. Read back: 1 when the lane path is in use  */
#define PAI_OPT_FIXED_BASE 5     /* 1 (default): PAI_OBF_RNG encryption with the private key set samples
                                    r^n through fixed bases (G_p^a_p, G_q^a_q: same distribution as
                                    r^n for uniform r, see pai_ctx_fixed_base_info); 0: r from the
                                    ChaCha20 stream and r^n by exponentiation. Read back: 1 when used */
#define PAI_OPT_FB_WINDOW 6      /* digit window of the fixed-base tables: 8, 12, 16 or 20 .. 24 bits (default 16, or
                                    $FLEXPAI_FB_WINDOW); setting it drops the tables (rebuilt lazily). Read
                                    back: the window of the resident tables, which is the largest one <= the
                                    requested window whose 2 K 2^W rows fit $FLEXPAI_FB_MAX_BYTES (default:
                                    free device memory less max(4 GiB, 1/12 of the device)).
                                    1024/2048-bit keys (Shoup rows): when that window is below the requested one,
                                    the exponent is cut unevenly if that saves a whole digit within the same
                                    budget -- the smallest digit count that fits, no digit wider than the request,
                                    the first few one bit wider than the rest (csrc/fb_cut.hpp; nb = 2048 on an
                                    idle MI355X, 23 requested: 12 digits of 23 bits + 34 of 22, 46 digits in 2 x
                                    109 GB instead of 47 in 2 x 88.3 GB). The window read back is then the
                                    narrower width (22), pai_ctx_fixed_base_info's digits the true count (46),
                                    pai_ctx_fixed_base_setup's bytes the true size. Ciphertexts do not depend on
                                    the cut. 4096-bit keys and the public tables keep the uniform cut.
                                    $FLEXPAI_FB_WINDOW=auto: a process holding ONE private key asks for 24 and
                                    gets the largest window whose tables fit $FLEXPAI_FB_AUTO_FRAC (default
                                    0.75) of the free memory (W = 22 at nb = 2048, 21 at nb = 4096 on an idle
                                    MI355X); a process holding several keys gets 16                          */
#define PAI_OPT_FB_READY 7       /* read-only: 1 when the fixed-base tables are resident                    */
#define PAI_OPT_FB_PAIR 8        /* read-only: limbs of p_h (19, 37; 76 for the 4096-bit pair-group tables)
                                    when the resident tables are pair tables (kernels_fbp.hpp,
                                    kernels_grp_pair.hpp: the default; round 1's k_fb / k_fbg were retired in round 6),
                                    else 0                                                                     */
#define PAI_OPT_PAIR 9           /* read-only: bit 0 = decryption, bit 1 = CRT encryption (stage B), bit 2 =
                                    public-key encryption (n of at most 1024 bits, of 1537..2048 bits, and, in a
                                    context without the private key, of 2049..4096 bits) run on p-adic pairs
                                    (kernels_pair.hpp, kernels_dec4.hpp, kernels_pe.hpp, kernels_pe1.hpp,
                                    kernels_pe4.hpp: the default; $FLEXPAI_PAIR=0 at context creation selects
                                    the kernels they replace); bit 3 = this context holds a private key of
                                    2049..4096 bits and its encryption above the rows (more than PAI_OPT_ROWS_MAX and
                                    more than PAI_OPT_CRT4_MIN elements, explicit r or device RNG without resident
                                    fixed-base tables) runs the split-pair CRT (kernels_crt4.hpp). A key holder's
                                    bit 2 stays 0 at 2049..4096 bits. Bit 2 says the constants are set up: of the
                                    1537..2048-bit keys only those of 128 ciphertext words (n of 2033..2048 bits)
                                    run k_pe_*, the others k_encrypt. The whole order: csrc/encrypt_route.hpp  */
#define PAI_OPT_PUBLIC_FB 10     /* 1 (default): PAI_OBF_RNG encryption WITHOUT the private key (2048-bit n) samples
                                  * r^n through the public fixed bases (kernels_pfb.hpp) once the break-even count
                                  * is reached (pai_ctx_public_fb_policy); get: 1 when the path is enabled and not
                                  * known unavailable                                                          */
#define PAI_OPT_PFB_READY 11     /* read-only: 1 when the public fixed-base tables are resident               */
#define PAI_OPT_PFB_WINDOW 12    /* digit window of the public tables: 12, 16 or 20 (the windows pinned to the
                                  * reference's goldens; default 16: 324 rows of 512 B per element, 10.9 GB of
                                  * tables; $FLEXPAI_FB_WINDOW=auto: 20 for a process with one context)       */
#define PAI_OPT_SPLIT_SAMPLER 13 /* read-only: bit 0 = the resident 4096-bit key-holder tables, bit 1 = the resident
                                  * public tables are sampled on split pairs (kernels_sgp.hpp: k_sgp, the default;
                                  * $FLEXPAI_SGP=0 at table build selects k_fbgp / k_pfb); bit 2 = the resident
                                  * 1024/2048-bit key-holder tables hold Shoup rows sampled on split pairs
                                  * (kernels_fbs.hpp: k_fbs, the default; $FLEXPAI_FBS=0 in the test build keeps
                                  * k_fbp's Montgomery rows); bit 3 = the resident 4096-bit key-holder tables add
                                  * Shoup rows (kernels_sgs.hpp: k_sgs, the default where they price lower than the
                                  * factored rows at their window; $FLEXPAI_SGS=0 keeps k_sgp, =1 takes them
                                  * whenever they fit)                                                        */
#define PAI_OPT_ROWS_MAX 14      /* calls of at most this many elements (default 4096) run their exponentiations with
                                  * each residue on a 16-lane row (kernels_crtw.hpp: the key holder's CRT encryption
                                  * k_crt_w and decryption k_dec_w, a public-key-only party's encryption k_pe_w; the
                                  * latency of protocol-sized calls) instead of one lane / lane pair each; 0
                                  * disables. Same bits either way. Where the rows stand in the order of encrypt
                                  * paths: csrc/encrypt_route.hpp                                                */
#define PAI_OPT_CRT4_MIN 15      /* a 2049..4096-bit key holder's calls of at most this many elements (default 128, one
                                  * block of lane pairs) that the rows do not take stay on the public-key kernel
                                  * instead of the split-pair CRT (kernels_crt4.hpp); 0: every such call runs the CRT.
                                  * Whether a lower floor would be faster has not been measured. Same bits either way
                                  * (the order of encrypt paths: csrc/encrypt_route.hpp)                         */
#define PAI_OPT_MATMUL_FUSED 16  /* 1 (default): pai_matmul[_dev] runs the fused windowed multi-exponentiation
                                  * (kernels_mm.hpp: k_mm_sign, k_mm_tab, k_mm_acc, then the k_add tree over the
                                  * ceil(K / 16) chunk partials) for the calls it was measured faster on: d >= 16 and
                                  * K m d of at least twice the chip's resident lane groups (131 072 terms at 1024 bits,
                                  * 65 536 at 2048, 32 768 at 4096 on an MI355X); 0: every call runs one k_mul
                                  * exponentiation per term (k, i, j), one batch inversion over the terms and the k_add
                                  * tree over all of them. Read back: 1 when the fused path is in use. Same bits either way */
#define PAI_OPT_MATMUL_PATH 17   /* read-only: the path of this context's last pai_matmul[_dev] call: 0 = none yet,
                                  * 1 = term path, 2 = fused                                                     */

#define PAI_OPT_OBF_CHUNK 18     /* elements per slice of an in-place pai_obfuscate_dev (default 262 144, at least 64): the
                                  * call keeps r^n of one slice in a buffer of the context. Same bits for every value */
#define PAI_OPT_SEGDOT_FUSED 20  /* 1 (default): pai_segment_dot[_dev] runs the fused windowed multi-exponentiation
                                  * (kernels_sd.hpp: k_sd_sign, k_mm_tab over the distinct ciphertexts of a block of
                                  * chunks, k_sd_acc, then the segmented add over the chunk partials) for the calls it was
                                  * measured faster on: at least 65 536 entries that reuse every table the blocks
                                  * build at least 16 times (1024 and 2048 bits on an MI355X; the
                                  * same constants at 4096 bits, unmeasured); 0: every call gathers its entries and runs k_mul,
                                  * one batch inversion and the segmented add over them. Same bits either way */
#define PAI_OPT_SEGDOT_PATH 21   /* read-only: the path of this context's last pai_segment_dot[_dev] call: 0 = none yet,
                                  * 1 = term path, 2 = fused                                                     */
#define PAI_OPT_POOL_FUSED 22    /* 1 (default): pai_encrypt[_dev] with PAI_OBF_POOL runs k_pool_enc (kernels_pool.hpp: the
                                  * half-width product a + n ((b + M a) mod n)); 0: k_pool_join, the PAI_OBF_NONE
                                  * encryption and k_obf_mul, the kernels pinned to the reference. Same bits either way */
#define PAI_OPT_SCAN_TILE 23     /* tile length of pai_cumsum[_dev]'s blocked path: 0 (default) automatic -- one tile per
                                  * resident lane group of the chip, no tile shorter than 8 elements, and row chains when
                                  * the rows alone fill the chip or are no longer than a tile; T > 0: tiles of T elements at
                                  * every level of the scan (T >= L: row chains). Same bits for every value */
#define PAI_OPT_SCAN_PATH 24     /* read-only: the path of this context's last pai_cumsum[_dev] call: 0 = none yet,
                                  * 1 = row chains, 2 = blocked scan                                             */
#define PAI_OPT_FOLD_ROWS 25     /* pai_pack_ciphertexts[_dev] and pai_repack[_dev]: 1 (default) automatic -- calls of at
                                  * most PAI_FOLD_ROWS_MAX_<key bits> outputs fold on 16-lane rows (k_pack_fold_w,
                                  * csrc/kernels_foldw.hpp), larger ones on lane groups (k_pack_fold); 0: never rows; 2:
                                  * rows wherever a row kernel exists (n^2 of 74, 148 or 296 limbs of 28 bits). A host-buffer
                                  * call decides once, by the outputs of the whole call, whatever its chunks. Same bits
                                  * for every value */
#define PAI_OPT_FOLD_PATH 26     /* read-only: the path of this context's last pai_pack_ciphertexts[_dev] or
                                  * pai_repack[_dev] call: 0 = none yet, 1 = lane groups, 2 = rows               */
/* The automatic choice of PAI_OPT_FOLD_ROWS: the largest output count at which the row kernel was more than 5 % faster
 * than the group kernel in the same-process A/B of tools/fold_ab.py on an MI355X (profiles/fold_ab.json),
 * per key size (n^2 of 74 / 148 / 296 limbs). 0: that key size stays on lane groups. Measured at 64, 1 024, 4 096, 16 384
 * and 65 536 outputs, rows / groups for pai_pack_ciphertexts and pai_repack alike: 0.24, 0.24, 0.26, 0.79, 1.47 at 1024
 * bits; 0.36, 0.36, 0.37, 1.16, 1.21 at 2048; 0.68, 0.68, 0.68, 1.12, 1.06 at 4096. */
#define PAI_FOLD_ROWS_MAX_1024 16384
#define PAI_FOLD_ROWS_MAX_2048 4096
#define PAI_FOLD_ROWS_MAX_4096 4096

/* Number of visible GPUs (0 when there is none or the runtime cannot start). */
int pai_device_count(int* count);
/* Free and total device memory of `device` (bytes). */
int pai_device_mem_info(int device, uint64_t* free_bytes, uint64_t* total_bytes);
int pai_ctx_create(const uint8_t* n_le, size_t n_bytes, int device, pai_ctx** out);
int pai_ctx_set_private(pai_ctx* ctx, const uint8_t* p_le, const uint8_t* q_le, size_t half_bytes);
void pai_ctx_destroy(pai_ctx* ctx);
/* Fixed-base tables live in device memory the library keeps when they are released (a window change, a context's
 * end): the next table build in the process maps it again instead of waiting for the driver to wipe released memory
 * (csrc/table_arena.hpp). It goes back to the driver when the process's last context is destroyed, or now with this
 * call (no context may be building tables concurrently). $FLEXPAI_TABLE_POOL=0: plain hipMalloc / hipFree. */
void pai_release_table_cache(void);
/* Encryption with the private key set uses CRT over p^2, q^2 (same ciphertext bits, ~4x fewer
 * multiply-accumulates; for keys of 2049..4096 bits on split pairs above PAI_OPT_ROWS_MAX and PAI_OPT_CRT4_MIN
 * elements, ~6x fewer); PAI_OPT_CRT_ENCRYPT = 0 forces the public-key kernel. */
int pai_ctx_set_option(pai_ctx* ctx, int option, int value);
int pai_ctx_get_option(const pai_ctx* ctx, int option, int* value);
/* With PAI_OPT_STAGE_TIMING on: kernel durations (ms) of the last encrypt call, summed over all its chunks
 * (a host-buffer call's chunks included; past 64 chunks the recorded ones are folded into running sums,
 * which waits for them), in launch order (CRT: stage A, stage B, finish -- for keys of 2049..4096 bits above the rows k_crt4_pre + k_crt4_a,
 * k_crt4_b, k_crt_fin; public key on pairs: k_pe_pre, k_pe_pow, k_pe_fin,
 * or k_pe4_pre, k_pe4_pow, k_pe4_fin for n of 2049..4096 bits without the private key; other public-key
 * paths: the one encrypt kernel). Waits for them. */
int pai_ctx_stage_times(pai_ctx* ctx, float* ms_out, int max_out, int* count);
/* key bits, 32-bit words per ciphertext (2*key_bits/32), words per plaintext (key_bits/32) */
int pai_ctx_info(const pai_ctx* ctx, int* key_bits, int* ct_words, int* pt_words);
const char* pai_last_error(void);
/* Fixed-base obfuscation parameters (PAI_OPT_FIXED_BASE): the bases g_p, g_q (generators of Z_p*,
 * Z_q*, p < q) with G_h = g_h^n mod h^2, the digit count K and the window W. Element i's exponent is
 * a_h = raw_h mod (h - 1), raw_h = the little-endian integer of the first max(bits(p-1), bits(q-1)) + 64
 * bits of the ChaCha20 stream (rng_key, counter 0.., nonce = (index lo, index hi, 0x66786230 + h));
 * r^n mod h^2 is G_h^a_h, i.e. the ciphertext is the reference's encryption under the obfuscator
 * r = CRT(g_p^a_p mod p, g_q^a_q mod q). Builds the tables if they are not resident (like
 * pai_ctx_fixed_base_prepare); PAI_ERR_KEY with the reason when the path is unavailable.          */
int pai_ctx_fixed_base_info(pai_ctx* ctx, uint32_t* g_p, uint32_t* g_q, int* digits, int* window);
/* Build the fixed-base tables now (otherwise on the first PAI_OBF_RNG encryption with the private key).
 * 0 when they are resident; PAI_ERR_KEY / PAI_ERR_NOPRIV with the reason otherwise (encryption then
 * uses the generic CRT path; decryption is never affected).                                       */
int pai_ctx_fixed_base_prepare(pai_ctx* ctx);
/* Cost of the last table build: host ms (bases, B_k, constants, hipMalloc), device ms (table kernels),
 * resident table bytes.                                                                            */
int pai_ctx_fixed_base_setup(const pai_ctx* ctx, float* host_ms, float* device_ms, uint64_t* table_bytes);
/* Fixed-base break-even: a device-RNG encryption builds the tables only once the device-RNG
 * elements encrypted under this context (the current call included) reach `threshold` (estimated build
 * time / per-element saving against the generic path; $FLEXPAI_FB_MIN_ELEMS overrides); smaller calls
 * take the generic path (same ciphertext distribution). `seen`: elements counted so far. threshold = 0
 * once the tables are resident or known unavailable. Replaces nothing in the reference (its obfuscator,
 * obfuscator.py:23-37, has no per-key state); protects re-keying callers (he_sa_ft/train.py:39-40).  */
int pai_ctx_fixed_base_policy(pai_ctx* ctx, long long* seen, long long* threshold);

/* Public-key fixed bases (DESIGN.md §3 "Fixed bases without the private key"; replaces, for a party holding
 * only n, the per-element gmpy2.powmod(r, n, n^2) of obfuscator.py:35-36). The context draws 33 bases
 * g_0..g_32 in [2, n) from the OS CSPRNG (g_0 with Jacobi symbol (g_0 | n) = -1); element i's obfuscator is
 * r = prod_j g_j^e_j mod n with the exponents read from its ChaCha20 stream (rng_key, counter 0.., nonce =
 * (index lo, index hi, 0x70666230)) cut into W-bit digits: digits [0, K0) are e_0 (K0 = ceil((nb + 64) / W)),
 * then 32 runs of KS = ceil(96 / W) digits are e_1..e_32, each little-endian. The ciphertext is the
 * reference's encryption of x under that r.                                                            */
int pai_ctx_public_fb_prepare(pai_ctx* ctx);
/* Use these bases (nbases = 33, each base_bytes little-endian, 1 < g < n) instead of random ones; drops
 * resident public tables (rebuilt lazily). For reproducible runs and the parity tests. PAI_ERR_ARG unless
 * every base is a unit mod n, the bases are distinct and g_0 has Jacobi symbol (g_0 | n) = -1: the
 * conditions of the distribution argument that a caller can check.                      */
int pai_ctx_public_fb_set_bases(pai_ctx* ctx, const uint8_t* bases_le, size_t base_bytes, int nbases);
/* The resident public tables' bases (nbases x base_bytes, nullable), digit count K, window W, and K0.
 * PAI_ERR_KEY when the tables are not resident.                                                        */
int pai_ctx_public_fb_info(pai_ctx* ctx, uint8_t* bases_le, size_t base_bytes, int* nbases, int* digits,
                           int* window, int* e0_digits);
/* Break-even of the public tables, like pai_ctx_fixed_base_policy ($FLEXPAI_PFB_MIN_ELEMS overrides).  */
int pai_ctx_public_fb_policy(pai_ctx* ctx, long long* seen, long long* threshold);

/* Encrypt N plaintexts. dtype PAI_F32/F64/I64. obf_mode PAI_OBF_*.
 *   r_le:      PAI_OBF_GIVEN only: r values as little-endian byte strings of r_bytes each, element i
 *              at r_le + i*r_stride_bytes (stride 0 = the same r for every element). 1 <= r < n^2.
 *   rng_key32: PAI_OBF_RNG only: 32-byte ChaCha20 key; element i uses nonce (index_base + i).
 * Outputs: ct_out N*W words, exp_out N exponents, status_out N statuses (nullable).           */
int pai_encrypt(pai_ctx* ctx, int dtype, const void* x, size_t N, int exp_mode, int32_t fixed_exp,
                int obf_mode, const uint8_t* r_le, size_t r_stride_bytes, size_t r_bytes,
                const uint8_t* rng_key32, uint64_t index_base,
                uint32_t* ct_out, int32_t* exp_out, int32_t* status_out);

/* k-way homomorphic add: out_i = prod_j ct_j,i^(16^(E_i - e_j,i)) mod n^2, E_i = max_j e_j,i. */
int pai_add(pai_ctx* ctx, const uint32_t* const* cts, const int32_t* const* exps, int k, size_t N,
            uint32_t* ct_out, int32_t* exp_out);

/* Re-randomise N ciphertexts: ct_out_i = ct_i * r_i^n mod n^2 (apply_obfuscation, obfuscator.py:23-37, over an array).
 * obf_mode is PAI_OBF_GIVEN (r_le, r_stride_bytes, r_bytes as for pai_encrypt) or PAI_OBF_RNG (rng_key32; element i
 * uses the global index index_base + i); PAI_OBF_NONE is PAI_ERR_ARG. Exponents are not touched and not passed.
 * Inputs must be < n^2, as for pai_add. ct_out may be ct.
 *
 * The bits contract: out[i] = ct[i] * E0[i] mod n^2, where E0 is what pai_encrypt_dev writes for N int64 zeros
 * (PAI_EXP_AUTO) on the same context state with the same obf_mode, r, rng key, index_base and N. The call takes the
 * route of that encryption (csrc/encrypt_route.hpp): it counts its N elements towards the same break-even counters
 * (pai_ctx_fixed_base_policy, pai_ctx_public_fb_policy), builds the same tables and draws the same r per global
 * element index. The sampler is decided once per call, for all N, so the bits depend neither on PAI_OPT_OBF_CHUNK nor
 * on the host-buffer call's chunks; a call cut in two by the caller (index_base advanced by the first part's count)
 * gives the same bits whenever both parts meet the same sampler (tables resident, or never wanted). */
int pai_obfuscate(pai_ctx* ctx, const uint32_t* ct, size_t N, int obf_mode,
                  const uint8_t* r_le, size_t r_stride_bytes, size_t r_bytes,
                  const uint8_t* rng_key32, uint64_t index_base, uint32_t* ct_out);

/* Decrypt + decode. val_out: float64 value (status OK/INT), mant_out: signed mantissa when it
 * fits int64 (nullable), status_out (required), raw_out: N * pt_words canonical plaintexts
 * m = D(c) in [0, n) (nullable).
 * exp: any int32 (it arrives from a peer); the decode follows FixedPointNumber.decode over the whole range and never
 * forms 4 * exp where that would wrap. For exp > 0 the value is float(M) * 16^-exp in double arithmetic: a denormal
 * factor for exp = 256 .. 268 and 0.0 from exp = 269 on, so the result is +-0.0 with the mantissa's sign there
 * (PAI_EL_FLOAT_OVF first, if |M| >= 2^1024 - 2^970). For exp <= 0 the result is the integer M * 16^-exp: PAI_EL_INT
 * with mant_out while it has at most 63 bits (so -2^63 is PAI_EL_INT_BIG), which no M but 0 has from exp = -16 down;
 * M = 0 is PAI_EL_INT 0 at every exp <= 0. val_out of a PAI_EL_INT_BIG element is the nearest double, +-inf beyond.  */
int pai_decrypt(pai_ctx* ctx, const uint32_t* ct, const int32_t* exp, size_t N, double* val_out,
                int64_t* mant_out, int32_t* status_out, uint32_t* raw_out);

/* Ciphertext x plaintext, element-wise: out_i = ct_i (x) x_(i*x_stride) (x_stride 0: one scalar for all,
 * 1: one per element), x of dtype PAI_F32/F64/I64 encoded like FixedPointNumber.encode; exponent
 * exp_i + e(x). Negative scalars: invert(ct)^|m|, computed as ONE batch inversion for the array.
 * status_out (nullable): PAI_EL_ENC_RANGE where the scalar does not fit the 64-bit encoder.      */
int pai_mul(pai_ctx* ctx, const uint32_t* ct, const int32_t* exp, size_t N, int dtype, const void* x, size_t x_stride,
            uint32_t* ct_out, int32_t* exp_out, int32_t* status_out);
/* Ciphertext + plaintext, element-wise: out_i = ct_i (+) x_(i*x_stride), x encoded like
 * FixedPointNumber.encode(x, max_exponent=exp_i) (fixedpoint_number.py:81-84) and raw-encrypted with r = 1,
 * exponent max(exp_i, e(x)). status_out (nullable): PAI_EL_FLOAT_OVF where x * 16^E is not a finite double
 * (OverflowError), PAI_EL_ENC_RANGE where |M| >= 2^(nb-3) (the exact |M| > max_int test is the caller's);
 * those outputs are undefined and the caller redoes them. Integers are exact (numpy's object add loop sees
 * Python ints), so int64 * 16^E never wraps. */
int pai_add_plain(pai_ctx* ctx, const uint32_t* ct, const int32_t* exp, size_t N, int dtype, const void* x,
                  size_t x_stride, uint32_t* ct_out, int32_t* exp_out, int32_t* status_out);
/* Segmented k-way add: out_s = prod over t in [seg_off[s], seg_off[s+1]) of ct[index[t]] aligned to the
 * segment's maximum exponent (same as pai_add over the members). index and seg_off (nseg + 1 offsets,
 * seg_off[0] = 0, non-decreasing) are host arrays in both variants. An empty segment yields ciphertext 1
 * with exponent INT32_MIN. The _dev variant synchronises `stream` once per reduction level. */
int pai_segment_add(pai_ctx* ctx, const uint32_t* ct, const int32_t* exp, size_t N, const int64_t* index,
                    const int64_t* seg_off, size_t nseg, uint32_t* ct_out, int32_t* exp_out);
/* Segmented weighted sum, the sparse encrypted-by-plain product: out_s = sum over t in [seg_off[s], seg_off[s+1]) of
 * ct[index[t]] (x) x[t]. index holds nnz = seg_off[nseg] entries in [0, N) and may repeat an entry inside a segment and
 * across segments; seg_off holds nseg + 1 non-decreasing offsets, seg_off[0] = 0; both are host arrays in both variants,
 * as for pai_segment_add. x holds nnz scalars of PAI_F32 / PAI_F64 / PAI_I64 aligned with index (a device pointer in the
 * _dev variant). A bad index, a decreasing offset or a null pointer is PAI_ERR_ARG before any launch.
 *   Term t of segment s is ct[index[t]] (x) x[t] exactly as pai_mul forms it: FixedPointNumber.encode of the scalar,
 *   invert(ct) for a negative mantissa, exponent exp[index[t]] + e(x[t]). The terms of a segment are summed with
 *   __add__'s alignment to the segment's largest exponent; stored zeros count towards that maximum, as in pai_matmul.
 *   An empty segment yields ciphertext 1 with exponent INT32_MIN. ct_out and exp_out equal, bit for bit, pai_mul over
 *   the gathered entries followed by pai_segment_add over consecutive ranges, entries whose scalar does not encode
 *   included (the factor 1); status_out (nullable, nnz entries) holds pai_mul's statuses. A ciphertext without inverse
 *   mod n^2 that meets a negative scalar ends the call with PAI_ERR_NOINV. The output is not re-randomised.
 * PAI_OPT_SEGDOT_FUSED / PAI_OPT_SEGDOT_PATH: window tables are built once per distinct ciphertext that a block of
 * chunks (16 consecutive entries of one segment) references, so the cost follows the stored entries; same bits on
 * either path. The _dev variant synchronises `stream` (sign flags, batch inversion, every level of the segmented add). */
int pai_segment_dot(pai_ctx* ctx, const uint32_t* ct, const int32_t* exp, size_t N, const int64_t* index,
                    const int64_t* seg_off, size_t nseg, int dtype, const void* x, uint32_t* ct_out, int32_t* exp_out,
                    int32_t* status_out);
/* Encrypted histogram: the per-cell sums of N ciphertexts over an [N][F] matrix of bin ids (row-major, bin_stride >= F
 * elements per row, PAI_BIN_U8 or PAI_BIN_U16) and an optional node id per sample (node nullable: every sample in node
 * 0, nodes must be 1). Cell (v, f, b) has index (v F + f) B + b and sums the samples i with node[i] == v and
 * bins[i][f] == b; no index list exists on the host (per-bin sums of all features of IV_FFS at once, and the
 * (node, feature, bin) sums of encrypted g and h in gradient boosting).
 *   A sample with node[i] < 0 or node[i] >= nodes is in no cell, and a bin id >= B is in no cell of that feature (a
 *   "missing" value); neither is an error. ct_out / exp_out of a cell equal pai_segment_add over the cell's members bit
 *   for bit (prod c_i^(16^(E - e_i)) mod n^2, canonical, E the cell's largest exponent), whatever the order of the
 *   members, the runs, the feature blocks or the host variant's chunks. An empty cell yields ciphertext 1 with exponent
 *   INT32_MIN. count_out (nullable, nodes F B entries) holds the members per cell. The output is not re-randomised; the
 *   call needs the public key only.
 *   PAI_ERR_ARG before any launch: a null pointer, bin_stride < F, F = 0, B = 0 or B above 256 (u8) / 65536 (u16),
 *   nodes = 0, nodes F B above 2^24 cells, N F at or above 2^31.
 * Members of a cell are summed in runs of PAI_HIST_RUN by k_hist_acc, which reads the member lists built on the device,
 * and the runs' partials by the segmented add. The features are processed in blocks whose member lists fit a scratch
 * budget of the context (256 MiB). The host-buffer variant moves the samples in chunks of 65536 and combines the chunks'
 * cell sums with one k-way add.
 * The _dev variant (device pointers for ct, exp, bins, node and all outputs) takes the context lock and chains on the
 * previous call's event like every _dev call; it synchronises `stream` once to read the cell counts and then as often
 * as the closing pai_segment_add_dev over the partials (once per reduction level). */
enum { PAI_BIN_U8 = 0, PAI_BIN_U16 = 1 };
#define PAI_HIST_RUN 64
int pai_histogram(pai_ctx* ctx, const uint32_t* ct, const int32_t* exp, size_t N, int bin_dtype, const void* bins,
                  size_t F, size_t bin_stride, const int32_t* node, size_t nodes, size_t B, uint32_t* ct_out,
                  int32_t* exp_out, int64_t* count_out);
/* pai_histogram over a sparse bin matrix, at a cost that follows the stored entries. The matrix is CSR: indptr holds
 * N + 1 offsets that start at 0 and never decrease, indices the feature of every stored entry (inside [0, F), strictly
 * increasing inside a row), data its bin id (PAI_BIN_U8 / PAI_BIN_U16). Every (i, f) that is not stored has bin
 * default_bin[f]; a default_bin[f] outside [0, B) puts the unstored entries of that feature in no cell. A stored bin id
 * >= B is a missing value, in no cell. node, nodes, B, the cell index (v F + f) B + b, the treatment of node ids outside
 * [0, nodes), the empty cell (ciphertext 1, INT32_MIN) and count_out are those of pai_histogram. N F is not limited.
 *   With z = default_bin[f]: a cell (v, f, b), b != z, holds exactly what pai_histogram gives on the densified matrix.
 *   The default cell (v, f, z) is T_v - S_{v,f}: T_v the sum of all samples of node v (pai_segment_add, once per
 *   call), S_{v,f} the sum of the stored entries of (v, f) whose bin is not z, stored missing values included
 *   (pai_segment_add), and `-` the ciphertext difference T_v * invert(S)^(16^(E_T - E_S)) mod n^2 of pai_mul by -1 and
 *   pai_add, bit for bit. Its exponent is E_T, the node's largest, and its ciphertext is the dense cell's raised to
 *   16^(E_T - E_cell): the same plaintext, and THE SAME BITS AS pai_histogram WHENEVER THE EXPONENTS OF A NODE ARE
 *   UNIFORM (int64 labels, fixed-exponent g / h, every packed buffer). Where nothing but default entries is stored for
 *   (v, f) the cell is T_v's bits and nothing is inverted; where count(v) equals the stored non-default entries it is
 *   the empty cell. count_out of a default cell is count(v) minus the stored non-default entries of (v, f). An S without
 *   inverse mod n^2 ends the call with PAI_ERR_NOINV. The output is not re-randomised; the call needs the public key
 *   only. Runs, feature blocks and the host variant's chunks change no bit, the default cells included: the
 *   subtraction happens once, on the combined slot sums.
 *   PAI_ERR_ARG before any ciphertext work: a null pointer, F = 0, B = 0 or B above the type's range, nodes = 0, nodes F B
 *   above 2^24, N or nnz at or above 2^31, an indptr that decreases or does not start at 0, an index outside [0, F), a row
 *   whose indices are not strictly increasing (the last two are found on the device by the counting pass).
 * Kernels (csrc/kernels_shist.hpp): the counting and the scattering pass run over tiles of stored entries, with the
 * tile's touched slots in an LDS hash table; the member lists then take pai_histogram's path (k_hist_acc, segmented
 * add). The _dev variant (device pointers for everything) synchronises `stream` to read nnz, to read the counts, per
 * level of the segmented add and for the batch inversion. */
int pai_histogram_sparse(pai_ctx* ctx, const uint32_t* ct, const int32_t* exp, size_t N, const int64_t* indptr,
                         const int32_t* indices, int bin_dtype, const void* data, size_t F, const int32_t* default_bin,
                         const int32_t* node, size_t nodes, size_t B, uint32_t* ct_out, int32_t* exp_out,
                         int64_t* count_out);
/* Prefix sums of a ciphertext array along one axis. The array is C-contiguous [outer][L][inner] (element (o, j, i) at
 * index (o L + j) inner + i, numpy's axis convention: no caller transposes). For every (o, i) and every j
 *     E_j   = max over j' <= j of e_j'                               (entries with exponent INT32_MIN skipped)
 *     out_j = prod over j' <= j of c_j'^(16^(E_j - e_j')) mod n^2     (canonical, < n^2)
 * which equals pai_add / pai_segment_add over the members of the prefix bit for bit, with that call's exponent rule.
 * PAI_SCAN_REVERSE scans from j = L - 1 downwards (suffix sums). An entry with exponent INT32_MIN (what
 * pai_segment_add and pai_histogram emit for an empty segment, with ciphertext 1) is the identity: it never enters the
 * maximum and no alignment is formed from it; a prefix of such entries only is ciphertext 1 with exponent INT32_MIN.
 * Inputs must be < n^2, as for pai_add. The output is not re-randomised; the call needs the public key only.
 *   outer, L or inner equal to 0: PAI_OK, nothing written. PAI_ERR_ARG before any launch: a null pointer with a
 *   non-empty array, unknown flag bits, outer L inner at or above 2^31, an output that overlaps the input.
 * Kernels (csrc/kernels_scan.hpp): k_scan runs one sequential chain per lane group, two Montgomery products per
 * element on rows of one exponent. Many short rows take one chain per (o, i) row; few long rows are cut into tiles
 * (PAI_OPT_SCAN_TILE): tile totals, a scan of the totals (recursively), then one chain per tile from its carry.
 * PAI_OPT_SCAN_PATH reports the path. Every tiling gives the same bits.
 * The host-buffer variant moves whole `outer` indices in slices of at most 1 GiB of ciphertext (one index at least) and
 * never cuts L or inner, so a slice holds whole rows and the bits do not depend on the slices.
 * The _dev variant (device pointers) takes the context lock and chains on the previous call's event like every _dev
 * call; it never synchronises `stream` itself (no host read-back: launches only). On the blocked path the context's
 * scratch buffer for the tiles' totals is freed and allocated again whenever a call needs more of it than any call
 * before, and that allocation synchronises the device. */
enum { PAI_SCAN_REVERSE = 1 };
int pai_cumsum(pai_ctx* ctx, const uint32_t* ct, const int32_t* exp, size_t outer, size_t L, size_t inner, int flags,
               uint32_t* ct_out, int32_t* exp_out);
/* Encrypted (m x K, row-major ciphertexts + exponents) times plain (K x d, row-major, dtype as above):
 * out[i][j] = sum_k ct[i][k] (x) x[k][j] with the reference's exponent alignment (bit-identical to
 * numpy's object dot over PaillierEncryptedNumber, whose sums are order independent). By default a product of
 * d >= 16 columns that fills the chip computes every output as a fused multi-exponentiation over chunks of 16 k
 * (PAI_OPT_MATMUL_FUSED; PAI_OPT_MATMUL_PATH reports the path taken): window tables of the m K ciphertexts, and of the inverses of those in a row k of x that holds a negative
 * scalar, are built once and shared by the d columns. A ciphertext without inverse mod n^2 in such a row ends the call
 * with PAI_ERR_NOINV, as on the term path. */
int pai_matmul(pai_ctx* ctx, const uint32_t* ct, const int32_t* exp, size_t m, size_t K, int dtype, const void* x,
               size_t d, uint32_t* ct_out, int32_t* exp_out);

/* Device-resident variants (device pointers, asynchronous on `stream`, a hipStream_t; pai_mul_dev and
 * pai_matmul_dev synchronise `stream` once, for the single host-side inversion of the batch; the fused pai_matmul_dev
 * synchronises once to read which rows of x hold a negative scalar, and a second time, for the inversion, only when
 * one does). pai_encrypt_dev never
 * waits on the host: the public-key chain's batch inversion (chunks of >= 16384 elements) inverts its one top value
 * in a host function queued on `stream` (hipLaunchHostFunc), so the call stays asynchronous and capturable; only
 * the first device-RNG call that BUILDS a key's fixed-base tables synchronises the device (per-key setup). */
int pai_encrypt_dev(pai_ctx* ctx, int dtype, const void* d_x, size_t N, int exp_mode, int32_t fixed_exp,
                    int obf_mode, const uint32_t* d_r_words, size_t r_stride_words, size_t r_words,
                    const uint8_t* rng_key32, uint64_t index_base,
                    uint32_t* d_ct, int32_t* d_exp, int32_t* d_status, void* stream);
/* d_cts: k consecutive [N][W] ciphertext arrays; d_exps: k consecutive [N] exponent arrays. */
int pai_add_dev(pai_ctx* ctx, const uint32_t* d_cts, const int32_t* d_exps, int k, size_t N,
                uint32_t* d_out, int32_t* d_exp_out, void* stream);
int pai_decrypt_dev(pai_ctx* ctx, const uint32_t* d_ct, const int32_t* d_exp, size_t N, double* d_val,
                    int64_t* d_mant, int32_t* d_status, uint32_t* d_raw, void* stream);
/* pai_obfuscate on device buffers (r as for pai_encrypt_dev); the bits contract above. d_out == d_ct re-randomises in
 * place, in slices of PAI_OPT_OBF_CHUNK elements; a d_out that does not overlap d_ct receives r^n first and the
 * product over it, with no further buffer; a partial overlap is PAI_ERR_ARG. As asynchronous as pai_encrypt_dev. */
int pai_obfuscate_dev(pai_ctx* ctx, const uint32_t* d_ct, size_t N, int obf_mode,
                      const uint32_t* d_r_words, size_t r_stride_words, size_t r_words,
                      const uint8_t* rng_key32, uint64_t index_base, uint32_t* d_out, void* stream);
int pai_mul_dev(pai_ctx* ctx, const uint32_t* d_ct, const int32_t* d_exp, size_t N, int dtype, const void* d_x,
                size_t x_stride, uint32_t* d_out, int32_t* d_exp_out, int32_t* d_status, void* stream);
int pai_add_plain_dev(pai_ctx* ctx, const uint32_t* d_ct, const int32_t* d_exp, size_t N, int dtype,
                      const void* d_x, size_t x_stride, uint32_t* d_out, int32_t* d_exp_out, int32_t* d_status,
                      void* stream);
int pai_segment_add_dev(pai_ctx* ctx, const uint32_t* d_ct, const int32_t* d_exp, size_t N, const int64_t* index,
                        const int64_t* seg_off, size_t nseg, uint32_t* d_out, int32_t* d_exp_out, void* stream);
int pai_matmul_dev(pai_ctx* ctx, const uint32_t* d_ct, const int32_t* d_exp, size_t m, size_t K, int dtype,
                   const void* d_x, size_t d, uint32_t* d_out, int32_t* d_exp_out, void* stream);
int pai_segment_dot_dev(pai_ctx* ctx, const uint32_t* d_ct, const int32_t* d_exp, size_t N, const int64_t* index,
                        const int64_t* seg_off, size_t nseg, int dtype, const void* d_x, uint32_t* d_out,
                        int32_t* d_exp_out, int32_t* d_status, void* stream);
int pai_histogram_dev(pai_ctx* ctx, const uint32_t* d_ct, const int32_t* d_exp, size_t N, int bin_dtype,
                      const void* d_bins, size_t F, size_t bin_stride, const int32_t* d_node, size_t nodes, size_t B,
                      uint32_t* d_out, int32_t* d_exp_out, int64_t* d_count_out, void* stream);
int pai_histogram_sparse_dev(pai_ctx* ctx, const uint32_t* d_ct, const int32_t* d_exp, size_t N, const int64_t* d_indptr,
                             const int32_t* d_indices, int bin_dtype, const void* d_data, size_t F,
                             const int32_t* d_default_bin, const int32_t* d_node, size_t nodes, size_t B,
                             uint32_t* d_out, int32_t* d_exp_out, int64_t* d_count_out, void* stream);
int pai_cumsum_dev(pai_ctx* ctx, const uint32_t* d_ct, const int32_t* d_exp, size_t outer, size_t L, size_t inner,
                   int flags, uint32_t* d_out, int32_t* d_exp_out, void* stream);

/* Device-resident ciphertext buffers (csrc/engine_res.hip, kernels_res.hpp; no reference counterpart): memory for
 * the *_dev entry points that a caller without a HIP runtime of its own (the Python layer, which never imports torch)
 * can hold across calls, so that a chain of calls moves no ciphertext word over PCIe.
 *
 * Ownership: the blocks belong to a DEVICE, not to a context. A block outlives every context that wrote it and may be
 *   passed to any context on the same device. Nothing frees a block but pai_dev_free.
 *   pai_dev_alloc     `bytes` of device memory (at least 16), from the allocator of the call buffers: when the device
 *                     is full, released table memory (pai_release_table_cache) goes back to the driver first.
 *   pai_dev_free      A FREE THAT SYNCHRONISES: it waits for all work queued on the device (hipDeviceSynchronize) and
 *                     then frees, so dropping a block while kernels that read it are still queued is safe, on whatever
 *                     stream they were queued. Null is PAI_OK.
 *   pai_dev_upload    host -> device, pai_dev_download: device -> host. Complete on return. Each first waits for the
 *                     work queued on the device, so a download sees the result of every *_dev call made before it and
 *                     an upload never overwrites a block that a queued kernel still reads. They go through two pinned
 *                     staging slots of at most 64 MiB per device: the host threads (at most 16) fill or drain one slot
 *                     while the other crosses PCIe, the pattern of pai_add / pai_decrypt. Calls are serialised by one
 *                     mutex; a call that fails waits for its copies in flight before it returns. In the test build
 *                     $FLEXPAI_RES_SLOT (bytes) shrinks the slot.
 *   pai_dev_copy      device -> device, queued on the NULL stream and not waited for: ordered with *_dev calls made on
 *                     the null stream (the Python layer's), and complete before any pai_dev_free, pai_dev_upload or
 *                     pai_dev_download that follows, since those wait for the device.
 *   pai_dev_release_staging  gives the copy streams, events and pinned slots (up to 128 MiB of pinned host memory per
 *                     device) back now; the next transfer makes them again. Otherwise they live as long as the process.
 *   pai_dev_io_stats  process-wide bytes moved by pai_dev_upload and by pai_dev_download since the process started
 *                     (each nullable).
 *
 * pai_take_dev: out[j] = in[index[j]], words and exponents (kernels_res.hpp k_take). index holds M entries and is a
 *   HOST array, as in pai_segment_add_dev; an entry lies in [0, N) and may repeat, or is -1, which writes the identity
 *   the API uses for an empty segment: ciphertext 1, exponent INT32_MIN. PAI_ERR_ARG before any launch, with the output
 *   untouched: any other index value, a null pointer with M > 0, an output that overlaps the input. M = 0 is PAI_OK. Rows
 *   move as 16-byte vectors when ct_words is a multiple of 4 and both bases are 16-byte aligned, word by word otherwise
 *   (a 1035-bit key has 65 words). Takes the context lock and chains on the previous call's event like every _dev call;
 *   synchronises `stream` once, after the launch (the index is caller memory).
 * pai_check_below_dev: *first_bad = the smallest i with ct[i] >= n^2, or -1 (k_check_below: compared from the top limb;
 *   one read-back of one word; synchronises `stream`). The range check of a received ciphertext array, done where the
 *   array already is. */
int pai_dev_alloc(int device, size_t bytes, void** d_out);
int pai_dev_free(int device, void* d);
int pai_dev_upload(int device, void* d_dst, const void* src, size_t bytes);
int pai_dev_download(int device, void* dst, const void* d_src, size_t bytes);
int pai_dev_copy(int device, void* d_dst, const void* d_src, size_t bytes);
int pai_dev_io_stats(uint64_t* h2d_bytes, uint64_t* d2h_bytes);
int pai_dev_release_staging(void);
int pai_take_dev(pai_ctx* ctx, const uint32_t* d_ct, const int32_t* d_exp, size_t N, const int64_t* index, size_t M,
                 uint32_t* d_ct_out, int32_t* d_exp_out, void* stream);
int pai_check_below_dev(pai_ctx* ctx, const uint32_t* d_ct, size_t N, int64_t* first_bad, void* stream);

/* Index lists on the device (kernels_res.hpp k_check_idx, k_seg_offsets, k_seg_rows; no reference counterpart): the
 * take and the segment sums of above for a caller whose index is already device memory (a nonzero, an argsort, a
 * top-k selection made on the GPU). Semantics and bits are those of pai_take_dev / pai_segment_add_dev for the same lists.
 *
 * Operands: d_index (`M` resp. `total` int64 entries) and d_seg_off (nseg + 1 int64 words) are DEVICE memory. `total` is
 *   the number of index entries, which the caller knows from the index's size. An index entry lies in [0, N) and may
 *   repeat; for pai_take_idx_dev with allow_empty != 0 it may also be -1, which writes ciphertext 1 with exponent
 *   INT32_MIN. seg_off[0] == 0, offsets do not decrease, seg_off[nseg] == total. An empty segment gives ciphertext 1 with
 *   exponent INT32_MIN.
 * Validation runs on the device. d_bad names two device int64 words that the call sets:
 *     d_bad[0]  the smallest position whose index value is invalid, or -1;
 *     d_bad[1]  the smallest offending position of seg_off (0: seg_off[0] != 0; s + 1: seg_off[s + 1] < seg_off[s];
 *               nseg: seg_off[nseg] != total), or -1. pai_take_idx_dev leaves it -1.
 *   A check kernel runs first on `stream`; every kernel behind it reads d_bad first and returns without reading through
 *   the index and without writing when either word is >= 0. On bad lists the outputs are therefore UNTOUCHED and the call
 *   still returns PAI_OK: the caller reads the two words when it wants to know. PAI_ERR_ARG before any launch is kept for
 *   what the host can see: a null pointer with a non-zero count (d_bad and, for the segment sums, d_seg_off are always
 *   required), an output that overlaps an input, d_bad overlapping a list, N, M or total >= 2^40, nseg >= 2^30 or
 *   total / 16 + nseg >= 2^31.
 * No host wait: neither call synchronises a stream or the device, copies to the host, or allocates; scratch is the
 *   context's, sized from total and nseg alone. Both take the context lock and chain on the previous call's event like
 *   every _dev call, so they are asynchronous and capturable once the context's scratch has its size. The lists and
 *   d_bad must stay valid until the stream has run the call.
 * Levels: the host does not know the longest segment, so pai_segment_add_idx_dev runs the smallest l >= 1 with
 *   16^l >= total levels of the 16-way tree; a segment that is finished earlier passes through unchanged. */
int pai_take_idx_dev(pai_ctx* ctx, const uint32_t* d_ct, const int32_t* d_exp, size_t N, const int64_t* d_index, size_t M,
                     int allow_empty, uint32_t* d_ct_out, int32_t* d_exp_out, int64_t* d_bad, void* stream);
int pai_segment_add_idx_dev(pai_ctx* ctx, const uint32_t* d_ct, const int32_t* d_exp, size_t N, const int64_t* d_index,
                            size_t total, const int64_t* d_seg_off, size_t nseg, uint32_t* d_out, int32_t* d_exp_out,
                            int64_t* d_bad, void* stream);

/* Packed plaintexts: many signed fixed-point values per ciphertext (no reference counterpart; opt-in, both peers must
 * be flexpai; csrc/kernels_pack.hpp). Every packed ciphertext is an ordinary reference ciphertext
 * raw_encrypt(M mod n, pk, r), so pai_add, pai_mul by an integer and pai_obfuscate act on all slots at once.
 *
 * Layout (n of nb bits): slot_bits sb, a multiple of 8 in [16, 64]; 2 <= value_bits vb <= sb; 1 <= slots k <=
 *   floor((nb - 2) / sb); exponent e, the library's base-16 exponent (value = t * 16^-e). B = 2^sb. The bound on k
 *   keeps |M| < 2^(k sb - 1) <= 2^(nb - 3) < max_int = n / 3 - 1. Anything else is PAI_ERR_ARG.
 * Encode: value i of a call goes to ciphertext i / k, slot i % k (slot 0 least significant). t_i is the library's
 *   encoding at the fixed exponent e (pai_encrypt with PAI_EXP_FIXED: rint(ldexp(v, 4 e)) for floats, |v| < 1e-200 -> 0).
 *   A value with |t_i| > 2^(vb - 1) - 1 (NaN and +-inf among them) gets status PAI_EL_ENC_RANGE and is encoded as 0; its
 *   neighbours are untouched and the call succeeds. Slots past the last value are 0.
 * Plaintext: M_c = sum_j t_(c k + j) B^j, a SIGNED integer with signed digits; m_c = M_c mod n (negatives are
 *   n - |M_c|, the library's sign convention). No bias is added and no term count is needed at decode time.
 * Ciphertext: ct_c = (1 + n m_c) r_c^n mod n^2; r and index_base count CIPHERTEXTS. The bits contract, as for
 *   pai_obfuscate: ct_c = c0_c * E0_c mod n^2, where E0 is what pai_encrypt_dev writes for ceil(N / k) int64 zeros on the
 *   same context state with the same obf_mode, r, rng key and index_base: the same route (csrc/encrypt_route.hpp), the
 *   same break-even counters (counting ciphertexts, not values), the same tables, one sampler decision per call however
 *   the host-buffer call is chunked. PAI_OBF_NONE gives c0 itself.
 * Decode: m = D(ct), the raw plaintext of pai_decrypt. M = m if m <= max_int, m - n if m >= n - max_int, otherwise
 *   every value of that ciphertext gets PAI_EL_OVERFLOW. For j = 0 .. k-1: t_j = ((M + B/2) mod B) - B/2, M <- (M - t_j) / B;
 *   a non-zero M after k digits is PAI_EL_OVERFLOW for all its values too. Otherwise PAI_EL_OK, mant = t_j and
 *   val = (double)t_j * 2^(-4 e). Slot sums decode correctly while every slot keeps |sum t| <= 2^(sb - 1) - 1; an
 *   overflow from one slot into its neighbour cannot be seen in the plaintext (the Python layer keeps an exact bound).
 *
 * Outputs: ct_out ceil(N / slots) * W words; status_out N statuses (nullable on encrypt). pai_decrypt_packed without
 * the private key is PAI_ERR_NOPRIV. The device variants are as asynchronous as pai_encrypt_dev / pai_decrypt_dev and
 * keep their scratch in the context, like pai_obfuscate_dev; the host-buffer variants chunk like their neighbours. */
typedef struct { int32_t slot_bits, value_bits, exponent, slots; } pai_pack_layout;
int pai_pack_max_slots(const pai_ctx* ctx, int slot_bits, int* slots);   /* floor((key_bits - 2) / slot_bits) */
int pai_encrypt_packed(pai_ctx* ctx, int dtype, const void* x, size_t N, const pai_pack_layout* layout, int obf_mode,
                       const uint8_t* r_le, size_t r_stride_bytes, size_t r_bytes, const uint8_t* rng_key32,
                       uint64_t index_base, uint32_t* ct_out, int32_t* status_out);
int pai_encrypt_packed_dev(pai_ctx* ctx, int dtype, const void* d_x, size_t N, const pai_pack_layout* layout,
                           int obf_mode, const uint32_t* d_r_words, size_t r_stride_words, size_t r_words,
                           const uint8_t* rng_key32, uint64_t index_base, uint32_t* d_ct, int32_t* d_status,
                           void* stream);
int pai_decrypt_packed(pai_ctx* ctx, const uint32_t* ct, const pai_pack_layout* layout, size_t N, double* val_out,
                       int64_t* mant_out, int32_t* status_out);
int pai_decrypt_packed_dev(pai_ctx* ctx, const uint32_t* d_ct, const pai_pack_layout* layout, size_t N, double* d_val,
                           int64_t* d_mant, int32_t* d_status, void* stream);
/* Fold EXISTING ordinary ciphertexts into packed ones (FATE's cipher compression; csrc/kernels_pack.hpp k_pack_fold).
 * Needs the public key only. Value i of the N inputs (ct [N][W], exp [N]) goes to output i / k, slot i % k of the layout
 * (sb, vb, e = E, k), validated as above; ct_out holds ceil(N / k) * W words, status_out N statuses (nullable).
 * Shift: D_i = E - exp_i. Where 0 <= 4 D_i < sb the value contributes the factor ct_i^(16^D_i * 2^(sb j)): the reference's
 *   own alignment (increase_exponent_to) and the slot's place. exp_i = INT32_MIN (the ciphertext 1 of an empty segment of
 *   pai_segment_add) contributes the factor 1 with PAI_EL_OK. exp_i > E or 4 D_i >= sb is PAI_EL_ENC_RANGE: the factor is 1,
 *   the slot reads 0, its neighbours are untouched and the call succeeds. Slots past N are the factor 1.
 * Bits: out_c = product of the contributing factors mod n^2, canonical (below n^2): D(out_c) = sum_j t_j 16^D_j 2^(sb j)
 *   mod n, the plaintext pai_decrypt_packed decodes. For E = the largest exponent these are the bits of the reference's
 *   sum(c_j * (1 << (sb * j))) through PaillierEncryptedNumber.__mul__ and __add__. The output is a deterministic
 *   function of its inputs and is NOT re-randomised: pai_obfuscate does that afterwards. vb is not checked against the
 *   encrypted values, which the caller cannot see; the caller vouches that every slot keeps |t_j 16^D_j| <= 2^(sb - 1) - 1.
 * d_out overlapping d_ct is PAI_ERR_ARG. The _dev call never waits on the host (no inversion, no scratch: capturable),
 * takes the context lock and chains on the previous call's event like its neighbours; the host-buffer call chunks at
 * multiples of k values, like pai_encrypt_packed. Per output (k - 1) sb + 2 k + 1 products mod n^2 depend on each other, so a
 * call of few outputs is latency-bound, like one public exponentiation: such calls run the chain on 16-lane rows
 * (PAI_OPT_FOLD_ROWS), with the same bits. */
int pai_pack_ciphertexts(pai_ctx* ctx, const uint32_t* ct, const int32_t* exp, size_t N,
                         const pai_pack_layout* layout, uint32_t* ct_out, int32_t* status_out);
int pai_pack_ciphertexts_dev(pai_ctx* ctx, const uint32_t* d_ct, const int32_t* d_exp, size_t N,
                             const pai_pack_layout* layout, uint32_t* d_out, int32_t* d_status, void* stream);
/* Repack PACKED ciphertexts into fewer, fuller ones (SecureBoost+'s cipher compression on top of g/h packing: a
 * histogram cell carries 2 slots of the ~nb - 2 plaintext bits). Needs the public key only. The N inputs are packed
 * ciphertexts under in_layout = (sb, vb, e, s), validated as above; input j of output c is ct[c g + j], g = group >= 1
 * with s g <= floor((nb - 2) / sb). ct_out holds ceil(N / g) * W words under the layout (sb, vb, e, s g): value i of the
 * input buffer is value i of the output buffer (ciphertext i / (s g), slot i % (s g)).
 * Bits: out_c = prod_j ct[c g + j]^(2^(s sb j)) mod n^2, canonical (below n^2): the bits of the reference's
 *   sum(c_j * (1 << (s sb j))) through PaillierEncryptedNumber.__mul__ and __add__ at one exponent. A packed ciphertext
 *   encrypts the signed integer M_j, so the product encrypts sum_j M_j 2^(s sb j), the plaintext pai_decrypt_packed
 *   decodes under (sb, vb, e, s g); negative M_j work because m_j == M_j (mod n). Inputs past N are the factor 1. No
 *   exponents are passed; the output is NOT re-randomised (pai_obfuscate does that afterwards). The stride s sb is
 *   internal to this entry: a slot of any other entry stays at most 64 bits wide.
 * PAI_ERR_ARG before any launch: a null pointer, group < 1, an invalid in_layout, s g above the bound, an output that
 * overlaps the input. N = 0 is PAI_OK. The _dev call takes the context lock, chains on the previous call's event, never
 * waits on the host and needs no scratch; the host-buffer call chunks at multiples of g inputs. The kernel is
 * pai_pack_ciphertexts' (PAI_OPT_FOLD_ROWS / PAI_OPT_FOLD_PATH): (g - 1) s sb + 2 g + 1 dependent products per output. */
int pai_repack(pai_ctx* ctx, const uint32_t* ct, size_t N, const pai_pack_layout* in_layout, int group,
               uint32_t* ct_out);
int pai_repack_dev(pai_ctx* ctx, const uint32_t* d_ct, size_t N, const pai_pack_layout* in_layout, int group,
                   uint32_t* d_out, void* stream);

/* Obfuscator pool: r^n drawn ahead of time (no reference counterpart: the reference draws r and raises it to n inside
 * every encrypt, obfuscator.py:23-37). r^n does not depend on the plaintext, so a party draws obfuscators while it waits
 * for its peer and spends one per fresh ciphertext when the plaintext arrives: the online step is (1 + n m) rho mod n^2
 * alone (csrc/kernels_pool.hpp, DESIGN.md §5 "Pooled obfuscators"). The pool is a FIFO ring of ready obfuscators in device
 * memory, one per context, owned by the context.
 *
 *   pai_pool_reserve   (re)allocates the ring for `capacity` entries, dropping its contents; 0 frees it. 2 ceil(key bits
 *                      / 32) words per entry (the W words of a ciphertext; 512 MB per 2^20 entries at 2048 bits), from the
 *                      allocator of the call buffers: released table memory goes back to the driver first when the device
 *                      is full. Waits for the context's queued device work.
 *   pai_pool_fill[_dev] appends `count` entries. Entry j is, bit for bit, the E0 that pai_encrypt_dev writes for int64
 *                      zero at global index index_base + j with the same obf_mode (PAI_OBF_GIVEN or PAI_OBF_RNG; anything
 *                      else is PAI_ERR_ARG), r or rng key, on the same context state: the fill takes that encryption's
 *                      route (csrc/encrypt_route.hpp) and counts towards the same break-even counters, exactly as
 *                      pai_obfuscate does (one sampler decision per fill), so pooled ciphertexts have the distribution of
 *                      the party's ordinary ones. Arguments as for pai_encrypt / pai_encrypt_dev.
 *   pai_pool_put[_dev] appends caller-made rho rows [count][W], each < n^2 (the parity tests; obfuscators made on another
 *                      device). The caller vouches that they are n-th residues of uniform r; the arithmetic is right for
 *                      every rho < n^2.
 *   pai_pool_info      capacity, ready entries, entries taken over the context's life (each nullable).
 *
 * Ring limits: a fill or put of more than capacity - ready entries is PAI_ERR_ARG; nothing is appended and unconsumed
 *   entries are never overwritten. A take of more than `ready` (or without a ring) is PAI_ERR_ARG with both numbers in
 *   pai_last_error(); nothing is consumed. A host-buffer call checks its whole count before its first chunk.
 * Consumers: pai_encrypt[_dev] and pai_obfuscate[_dev] accept PAI_OBF_POOL; r and rng arguments are ignored. Element i
 *   of the call uses the entry at head + i, wrapping at capacity: out_i = (1 + n m_i) rho_i mod n^2, and ct_i rho_i mod
 *   n^2. Exponents and statuses are exactly those of the same call with PAI_OBF_NONE; an element whose status is not OK
 *   still consumes its entry. pai_encrypt_packed[_dev] with PAI_OBF_POOL is PAI_ERR_ARG.
 * Exactly once: a call advances the head under the context's mutex when it enqueues its work, and a call that fails
 *   after that point does not give entries back: two ciphertexts under one rho reveal the difference of their
 *   plaintexts ("Obfuscator keys").
 * Lifetime: pai_ctx_set_private (re-keying) and pai_ctx_destroy drop the pool.
 * Threads and streams: the rule of the other entry points holds -- calls on one context run one after the other, and a
 *   _dev call's stream first waits for the context's previous device work -- so a fill is complete before the take that
 *   follows it, on any stream. An encryption that arrives during a long fill therefore waits for it: fill in slices
 *   (the Python layer's prepare_obfuscators fills 65 536 entries per call). */
int pai_pool_reserve(pai_ctx* ctx, size_t capacity);
int pai_pool_fill(pai_ctx* ctx, size_t count, int obf_mode, const uint8_t* r_le, size_t r_stride_bytes, size_t r_bytes,
                  const uint8_t* rng_key32, uint64_t index_base);
int pai_pool_fill_dev(pai_ctx* ctx, size_t count, int obf_mode, const uint32_t* d_r_words, size_t r_stride_words,
                      size_t r_words, const uint8_t* rng_key32, uint64_t index_base, void* stream);
int pai_pool_put(pai_ctx* ctx, const uint32_t* rho, size_t count);
int pai_pool_put_dev(pai_ctx* ctx, const uint32_t* d_rho, size_t count, void* stream);
int pai_pool_info(pai_ctx* ctx, uint64_t* capacity, uint64_t* ready, uint64_t* taken_total);

/* Multi-GPU: ciphertext shards -> every rank (RCCL, opened with dlopen on first use; one process per GPU).
 * Rank 0 calls pai_comm_unique_id and hands the PAI_COMM_ID_BYTES bytes to the other ranks over any
 * channel; every rank then calls pai_comm_create (collective). */
#define PAI_COMM_ID_BYTES 128
int pai_comm_unique_id(uint8_t* id_out);
int pai_comm_create(const uint8_t* id, int world, int rank, int device, pai_comm** out);
void pai_comm_destroy(pai_comm* comm);
/* d_recv[r * bytes_per_rank ...] <- rank r's d_send; asynchronous on `stream` (a hipStream_t). */
int pai_allgather_dev(pai_comm* comm, const void* d_send, size_t bytes_per_rank, void* d_recv, void* stream);
/* Both halves of a ciphertext shard (words [n_per_rank][ct_words], exponents [n_per_rank]) in one grouped
 * launch: d_ct_all [world * n_per_rank][ct_words], d_exp_all [world * n_per_rank]. */
int pai_allgather_shards_dev(pai_comm* comm, const uint32_t* d_ct, const int32_t* d_exp, size_t n_per_rank,
                             int ct_words, uint32_t* d_ct_all, int32_t* d_exp_all, void* stream);

/* Key generation: the prime search on the device (csrc/engine_prime.hip, kernels_prime.hpp). These entry points take
 * no context -- a key does not exist yet -- but a device number; they are synchronous and keep one stream and one
 * scratch buffer per device for themselves. `bits` is the size of the primes: 256, 512, 1024 or 2048 (the halves of
 * 512- to 4096-bit keys); anything else is PAI_ERR_ARG. Integers are little-endian bytes.
 *
 * pai_next_prime: for each of the nstarts starts x (start_bytes each, bit `bits - 1` set, as getprimeover's
 * r | 1 << (bits - 1)) the smallest c > x that is divisible by no odd prime below 2000 and is a strong probable
 * prime to each of the first 40 odd primes -- gmpy_math.py:77-87's next_prime(r) as this package restates it.
 * The search goes window by window: the sieve's survivors in (x, x + window] meet base 3 in one launch for all
 * starts (pass 1), then each start's smallest survivor meets the other 39 bases in one launch (pass 2), the next
 * survivor if it fails, the next window when none is left. window = 0: the default, 4 * bits (5.8 mean prime gaps:
 * a window holds no prime with probability about e^-5.8 = 0.3 %). out_le: nstarts primes of start_bytes each;
 * passes_out (nullable): the windows used per start. A start whose window would cross 2^bits is not searched: its
 * output is zero, its passes_out is -1 and the call returns PAI_PRIME_OVERFLOW (the other starts are complete); the
 * caller searches that one on the host. */
#define PAI_PRIME_OVERFLOW 1
int pai_next_prime(int device, int bits, const uint8_t* starts_le, size_t start_bytes, size_t nstarts, uint32_t window,
                   uint8_t* out_le, int32_t* passes_out);
/* Kernel time (ms) and launches of pass 1 and of pass 2 in this thread's last pai_next_prime. */
int pai_prime_last_times(float* pass1_ms, float* pass2_ms, int* pass1_launches, int* pass2_launches);
/* verdict_u8[i * nbases + j] = 1 when candidate i (odd, bit `bits - 1` set) is a strong probable prime to base j:
 * with n - 1 = 2^s d, a^d is 1 or n - 1, or a^(2^r d) is n - 1 for some 0 < r < s. No sieving. Any uint32 base is
 * accepted, even ones and bases above 2^31 included; it is not reduced or checked against n. Base 0 gives 0 for every
 * candidate (0^d = 0 is neither 1 nor n - 1) and base 1 gives 1 for every candidate, as Python's pow does in the host's
 * test. At most 2^20 candidates and 2^12 bases per call. */
int pai_prime_test(int device, int bits, const uint8_t* cands_le, size_t cand_bytes, size_t ncand,
                   const uint32_t* bases_u32, size_t nbases, uint8_t* verdict_u8);
/* The sieve alone, on the host (no device): the offsets 0 < off <= window (0: the default) with x + off odd and
 * divisible by no odd prime below 2000, ascending. *count is their number; the first max_out are written.
 * PAI_PRIME_OVERFLOW when x + window reaches 2^bits. */
int pai_debug_prime_sieve(int bits, const uint8_t* x_le, size_t bytes, uint32_t window, uint32_t* offsets_out,
                          size_t max_out, size_t* count);

/* Debugging. Which kernels pai_encrypt[_dev] runs a call on is decided by one pure function of the facts below
 * (csrc/encrypt_route.hpp, which documents the order); this hook evaluates it and needs neither a context nor a
 * device. The library's other debugging hooks (pai_debug_fb_w, pai_debug_engine) are test interfaces and are not
 * declared here. */
typedef struct pai_route_facts {
  int has_priv;                       /* the private key is set */
  int crt_enabled, fb_enabled, pfb_enabled; /* PAI_OPT_CRT_ENCRYPT, PAI_OPT_FIXED_BASE, PAI_OPT_PUBLIC_FB */
  int crt_ok, crt_sa;                 /* 1024/2048-bit key holder: lane CRT constants, limbs of a prime (19 / 37) */
  int fbg_ok, rows_sa, crt4_ok;       /* 2049..4096-bit key holder: sampler constants, row limbs (74), k_crt4_* */
  int pe_ok, pe1_ok, pe4_ok, pew_ok;  /* public-key chains: k_pe_*, k_pe1_*, k_pe4_*, the k_pe_w op list */
  int pfb_supported;                  /* the public fixed-base kernels take this n */
  int ct_words;
  int rows_r_max;                     /* most words of r the 4096-bit rows stage */
  long long crtw_max, crt4_min;       /* PAI_OPT_ROWS_MAX, PAI_OPT_CRT4_MIN */
} pai_route_facts;
#define PAI_SAMPLER_NONE 0
#define PAI_SAMPLER_KEY 1      /* the key holder's fixed-base tables (pai_ctx_fixed_base_policy counts the call) */
#define PAI_SAMPLER_PUBLIC 2   /* the public fixed-base tables (pai_ctx_public_fb_policy counts the call) */
#define PAI_CHAIN_ENCRYPT 0    /* k_encrypt */
#define PAI_CHAIN_CRT_ROWS 1   /* k_crt_w, 1024/2048-bit key holder */
#define PAI_CHAIN_CRT_ROWS4 2  /* k_crt_w<74, 148>, 2049..4096-bit key holder */
#define PAI_CHAIN_CRT_LANE 3   /* k_crt_a, k_crt_b_pair */
#define PAI_CHAIN_CRT4 4       /* k_crt4_* */
#define PAI_CHAIN_PE_ROWS 5    /* k_pe_w */
#define PAI_CHAIN_PE 6         /* k_pe_* */
#define PAI_CHAIN_PE1 7        /* k_pe1_* */
#define PAI_CHAIN_PE4 8        /* k_pe4_* */
/* sampler: the tables the call is eligible for (used once wanted and built); chain: the per-element kernels otherwise */
int pai_debug_encrypt_route(const pai_route_facts* facts, int obf_mode, long long n, int r_words, int* sampler,
                            int* chain);

#ifdef __cplusplus
}
#endif
#endif /* FLEXPAI_H */
