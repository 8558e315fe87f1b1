/*
 * polar_mi355x.h -- C ABI of the MI355X (gfx950) SC / SC-list polar decoder library.
 *
 * This is the drop-in boundary for the hot path named in BASELINE.json: the Python decoder
 * modules (polar_amd.SC_Dec / SCL_Dec, mirroring the reference constructors and forward())
 * call these entry points through ctypes.  All pointers are device pointers unless a comment
 * says otherwise; the caller (PyTorch) owns every buffer; launches are asynchronous and
 * ordered on the given hipStream_t (passed as void*; NULL = legacy default stream).
 * No exceptions cross this boundary: 0 = success, negative = error, details from
 * pl_last_error_string() (thread-local).
 *
 * Alignment: every float, int32_t and double pointer needs only the natural alignment of its
 * element type (4, 4 and 8 bytes; a workspace holds fp64 tables and needs 8), and a uint8 output may
 * start at any address: a contiguous [bs, n] view that begins anywhere inside a larger buffer is a
 * valid argument.  A 16-byte aligned pointer only lets a kernel take its 16-byte load and store paths
 * (faster, same values).  The one exception is pl_scq_decode's llr_q, as stated there.
 *
 * Plans are device-bound: pl_plan_create allocates the plan's tables and loads its kernel module
 * on the device current at that call (hipSetDevice).  Decode/encode calls must pass a stream of
 * that device (or NULL with that device current); any other device gives PL_EINVAL.  Create one
 * plan per GPU to decode on several GPUs.
 *
 * Reference interfaces replaced (jaco267/polar-code-pytorch-sionna):
 *   pl_plan_create   SC_Dec.__init__   x_run_sn_polar/polar/polar_sc.py:10-32
 *                    SCL_Dec.__init__  x_run_sn_polar/polar/polar_scl.py:13-42
 *                    (my_sn/fec/polar/dec.py:18-31 and :183-242 for the exact-f variants)
 *   pl_sc_decode     SC_Dec.forward    x_run_sn_polar/polar/polar_sc.py:113-133
 *                    (f_mode=PL_F_EXACT: my_sn/fec/polar/dec.py:130-157)
 *   pl_plan_info / pl_plan_device: the plan's n, k, list size (polar_sc.py:14-17) and device
 *   pl_scl_decode    SCL_Dec.forward   x_run_sn_polar/polar/polar_scl.py:210-234
 *                    (+ final sorted msg_pm of _decode_np_batch :178-209)
 *   pl_hybrid_decode SCL_Dec(use_hybrid_sc=True).forward my_sn/fec/polar/dec.py:187, :497-498 (a stub
 *                    there: "not implement..."; the decoder its docstring cites)
 *   pl_crc_status    SCL_Dec(return_crc_status=True) my_sn/fec/polar/dec.py:534-535 (a stub there)
 *   pl_polar_encode  PolarEncoder.forward x_run_sn_polar/polar/enc.py:30-43
 *                    (butterfly form of my_sn/fec/polar/enc.py:85-96)
 *   pl_crc_attach    CRCEncoder.forward my_sn/fec/crc.py:85-104 (G-matrix CRC, 5G polynomials :38-52)
 *   pl_crc_check     CRCDecoder.forward my_sn/fec/crc.py:119-138 (re-encode, valid iff parity == 0)
 *   pl_gather_rows   Polar5GEncoder.forward rate matching c[:, ind_rate_matching]
 *                    my_sn/fec/polar/enc.py:378-392
 *   pl_rate_recover  Polar5GDecoder.forward rate recovery my_sn/fec/polar/dec.py:621-654
 *   pl_osd_plan_create OSDecoder.__init__ my_sn/fec/osd/dec.py:22-53
 *   pl_osd_decode    OSDecoder.forward  my_sn/fec/osd/dec.py:148-192 (_find_mrb :107-147, _find_min_dist :82-106)
 *   pl_bp_decode     the "iterative BP decoding" of my_sn/fec/polar/dec.py:1 and Polar5GDecoder's
 *                    dec_type "BP" (named there, not implemented)
 *   pl_scan_decode   no reference counterpart (soft-cancellation decoding with soft output; the contract is
 *                    stated below)
 *   pl_scf_decode    no reference counterpart (CRC-aided SC-Flip; the contract is stated below)
 *   pl_llr_quantize / pl_scq_decode: no reference counterpart (fixed-point SC on int8 LLRs; the contract
 *                    is stated below)
 *   pl_ae_decode     no reference counterpart (automorphism-ensemble SC; the contract is stated below)
 *   pl_pac_encode / pl_pac_decode: no reference counterpart (PAC codes: convolutional precoder and list
 *                    decoder; the contract is stated below)
 *   pl_pcl_table_create / pl_pcl_decode: no reference counterpart (list decoding under parity constraints
 *                    between the u-bits, "dynamic frozen bits"; the contract is stated below)
 *   pl_plan_kernel / pl_sc_specialize: no reference counterpart (kernel specialisation per
 *                    frozen set, the tree walk of polar_sc.py:54-98 resolved at compile time)
 */
#ifndef POLAR_MI355X_H
#define POLAR_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PL_OK 0
#define PL_EINVAL -1  /* bad argument / shape */
#define PL_EHIP -2    /* HIP runtime error */
#define PL_ENOTSUP -3 /* configuration not supported by this build */

#define PL_F_MINSUM 0 /* f = sign*sign*min(|x|,|y|) on clipped inputs (polar_sc.py:46) */
#define PL_F_EXACT 1  /* f = log(1+e^(x+y)) - log(e^x+e^y) (my_sn dec.py:39-43) */
#define PL_F_WIDE_RANGE 0x100 /* pl_sc_source / pl_sc_specialize: or-ed into PL_F_EXACT, the code object
                                 of plans whose llr_max exceeds 43 (full-range exp/log); without it,
                                 the code object of plans with llr_max <= 43 */

#define PL_PLAN_GENERIC 1u    /* pl_plan_create flag: never specialise the SC kernel */
#define PL_PLAN_CACHE_ONLY 2u /* pl_plan_create flag: use a cached specialised kernel, never compile */
#define PL_PLAN_FAST_SCL 4u   /* pl_plan_create flag (SCL): fast-SCL rate-0 / repetition pruning of
                                 my_sn/fec/polar/dec.py:367-376 (use with f_mode PL_F_EXACT for
                                 my_sn SCL_Dec semantics) */
#define PL_PLAN_JIT 8u        /* pl_plan_create flag (SC): compile a specialised kernel missing from
                                 the caches in this process (hiprtc, seconds); without it a cache
                                 miss runs the generic kernel */

#define PL_KERNEL_GENERIC 0     /* pl_plan_kernel kinds */
#define PL_KERNEL_SPECIALIZED 1
#define PL_KERNEL_SCL_SUBTREE 2 /* SCL plans: lane-per-path register-subtree kernel (default for
                                   2 <= L <= 32, 32 <= n <= 1024, no fast-SCL pruning) */

#define PL_OUT_F32 0  /* output 0.0f/1.0f floats, [bs, k] (reference output dtype) */
#define PL_OUT_U8 1   /* output 0/1 bytes, [bs, k] */

typedef struct pl_plan pl_plan;

/* Build an immutable decoding plan for a length-n polar code.
 * frozen_mask: HOST pointer to n bytes, nonzero = frozen position (frozen_pos of the reference).
 * list_size:   1 for SC plans; a power of two <= 32 for SCL plans.
 * f_mode:      PL_F_MINSUM or PL_F_EXACT.  llr_max: clipping bound (reference: 30; at most 700
 *              for list_size > 1, where log(1 + exp(llr_max)) must stay finite).
 * flags:       0, or PL_PLAN_GENERIC / PL_PLAN_CACHE_ONLY / PL_PLAN_JIT (/ PL_PLAN_FAST_SCL).
 *              An SC plan (list_size 1) runs a kernel specialised to its frozen set when a code
 *              object for it is cached ($PL_KERNEL_CACHE, <library dir>/kcache,
 *              ~/.cache/polar_mi355x; pl_sc_source + hipcc --genco, or pl_sc_specialize, put it
 *              there), otherwise the generic kernel (also exact).  PL_PLAN_JIT compiles a missing
 *              one in-process with hiprtc at plan creation (seconds; not in a process whose HIP
 *              runtime came with another ROCm's amd_comgr, e.g. torch's).  PL_SC_SPECIALIZE=0 in
 *              the environment selects the generic kernel.
 * n must be a power of two, 2 <= n <= 2048.  List plans: list_size <= 32 for n <= 1024,
 * list_size <= 16 at n = 2048 (the list state of one codeword must fit one CU's LDS); larger ones
 * are rejected here with PL_ENOTSUP. */
int pl_plan_create(pl_plan** out, int32_t n, const uint8_t* frozen_mask, int32_t list_size,
                   int32_t f_mode, float llr_max, uint32_t flags);
int pl_plan_destroy(pl_plan* plan);
/* n, k (information bits) and list size of a plan (any pointer may be NULL). */
int pl_plan_info(const pl_plan* plan, int32_t* n, int32_t* k, int32_t* list_size);
/* The HIP device the plan was created on (its tables and kernel module live there). */
int pl_plan_device(const pl_plan* plan, int32_t* device);

/* SC decode.  llr_logits: [bs, n] fp32 logits log(P(b=1)/P(b=0)) (NOT negated; the decoder
 * negates, polar_sc.py:122).  out_bits: [bs, k] decided information bits at info_pos ascending,
 * dtype per out_kind (PL_OUT_F32 / PL_OUT_U8). */
int pl_sc_decode(const pl_plan* plan, const float* llr_logits, int64_t bs, void* out_bits,
                 int32_t out_kind, void* hip_stream);

/* SCL decode.  out_pm (nullable): [bs, 2L] fp64, the reference's final sorted msg_pm.
 * workspace: device scratch of pl_scl_workspace_size(plan, bs) bytes -- the exact-f list kernels
 * keep path-independent caches of the upper tree there (22 KB per codeword at n = 1024, for at
 * most 16384 codewords: larger batches are decoded in chunks over it).  NULL with ws_bytes 0 runs
 * without them (same results, slower); a non-NULL workspace smaller than the size is PL_EINVAL. */
size_t pl_scl_workspace_size(const pl_plan* plan, int64_t bs);
int pl_scl_decode(const pl_plan* plan, const float* llr_logits, int64_t bs, void* out_bits,
                  int32_t out_kind, double* out_pm, void* workspace, size_t ws_bytes,
                  void* hip_stream);

/* Polar encoding with the plan's frozen set: u_bits [bs, k] fp32 0/1 -> codewords [bs, n] fp32. */
int pl_polar_encode(const pl_plan* plan, const float* u_bits, int64_t bs, float* codewords,
                    void* hip_stream);

/* CRC-aided SCL (my_sn/fec/polar/dec.py:507-518): after decoding, every path whose k decoded
 * bits fail the CRC (generator x^degree + sum of the bits of poly_mask, MSB-first shift register,
 * my_sn/fec/crc.py) gets +llr_max*k on its metric (the plan's llr_max; 30 in the reference,
 * dec.py:517) before the first argmin.  degree 0 turns it off.
 * Call before the plan's first decode.  Replaces SCL_Dec(crc_degree=...) (dec.py:210-218). */
int pl_plan_set_crc(pl_plan* plan, int32_t degree, uint32_t poly_mask);

/* Hybrid SC / SC-list decoding ([Cammerer_Hybrid_SCL]; SCL_Dec(use_hybrid_sc=True), which the
 * reference names and never implemented, my_sn/fec/polar/dec.py:187, :497-498): SC-decode every row
 * with sc_plan, list-decode with scl_plan only the rows whose SC result fails scl_plan's CRC.
 *   u_sc = SC(llr); ok = crc_valid(u_sc); rows = ascending indices where !ok;
 *   out = u_sc, out[rows] = SCL_crc(llr[rows]) exactly as pl_scl_decode decodes those rows;
 *   crc_ok = ok, crc_ok[rows] = crc_valid(out[rows]).
 * Not the same decoder as pure CRC-aided SCL: a row whose SC result passes the CRC keeps it, even
 * where the list decoder would pick another CRC-valid word.
 * sc_plan: list size 1; scl_plan: list size >= 2 with a CRC (pl_plan_set_crc; PL_ENOTSUP without);
 * both of the same n, k and frozen set and on the same device (PL_EINVAL otherwise).  Each plan
 * decodes with its own f mode, llr_max and kernel.
 * crc_ok (nullable): device [bs] bytes, 1 = the row's output passes the CRC.  list_rows (nullable):
 * device [bs] int32, its first *n_list entries receive the list-decoded rows, ascending.  n_list
 * (nullable): HOST pointer, their number.
 * workspace: device scratch of pl_hybrid_workspace_size(sc_plan, scl_plan, bs) bytes, required
 * (NULL or a smaller one is PL_EINVAL): 5 bytes per row for the flags and the row list, and one
 * chunk of min(bs, 16384) rows of LLRs, bits and the list plan's own workspace -- the failing rows
 * are gathered and list-decoded in chunks of that size, so this part does not grow with bs.
 * The call SYNCHRONISES its stream once: the number of failing rows sizes the list launches, so it
 * is read back (8 bytes) after the SC stage.  For the same reason it cannot be captured into a HIP
 * graph: on a capturing stream it returns PL_ENOTSUP before it touches the stream.  bs == 0 is PL_OK.
 * pl_crc_status: valid[b] = 1 iff the k bits of row b of bits ([bs, k], kind PL_OUT_F32 / PL_OUT_U8)
 * pass the plan's CRC (the last crc degree bits are the parity of the others), else 0; device [bs]
 * bytes.  PL_ENOTSUP for a plan without a CRC. */
size_t pl_hybrid_workspace_size(const pl_plan* sc_plan, const pl_plan* scl_plan, int64_t bs);
int pl_hybrid_decode(const pl_plan* sc_plan, const pl_plan* scl_plan, const float* llr_logits, int64_t bs,
                     void* out_bits, int32_t out_kind, uint8_t* crc_ok, int32_t* list_rows, int64_t* n_list,
                     void* workspace, size_t ws_bytes, void* hip_stream);
int pl_crc_status(const pl_plan* plan, const void* bits, int32_t kind, int64_t bs, uint8_t* valid,
                  void* hip_stream);

/* Which kernel a plan launches: *kind = PL_KERNEL_GENERIC / PL_KERNEL_SPECIALIZED (SC plans) or
 * PL_KERNEL_GENERIC / PL_KERNEL_SCL_SUBTREE (SCL plans; PL_PLAN_GENERIC or PL_SCL_TREE=0 in the
 * environment select the generic SCL kernel); path
 * (nullable) receives the code object file of a specialised kernel. */
int pl_plan_kernel(const pl_plan* plan, int32_t* kind, char* path, size_t path_len);

/* Compile (or find) the specialised SC kernel of a code into cache_dir (NULL = default cache)
 * without touching a GPU; path (nullable) receives the code object file.  Used to pre-build the
 * kernels of known codes.  f_mode: PL_F_MINSUM, PL_F_EXACT or PL_F_EXACT | PL_F_WIDE_RANGE (an
 * exact-f plan picks one of the two by its llr_max). */
int pl_sc_specialize(int32_t n, const uint8_t* frozen_mask, int32_t f_mode, const char* cache_dir,
                     char* path, size_t path_len);
/* The HIP source of the specialised SC kernel of a code and its cache file name (what
 * pl_sc_specialize would compile and look up), for compiling it out of process (hipcc --genco;
 * polar_amd/build.py).  *src_size = bytes needed including the NUL; src may be NULL. */
int pl_sc_source(int32_t n, const uint8_t* frozen_mask, int32_t f_mode, char* src, size_t src_len,
                 size_t* src_size, char* name, size_t name_len);

/* 5G NR data path (polar_amd/polar5g.py builds the tables on the host, 3GPP TS 38.212 5.4.1).
 * All pointers are device pointers; rows are contiguous fp32.
 * pl_crc_attach:   out[b] = [u[b], parity(u[b])], parity bit c = XOR of g_rows[m] bit c over the
 *                  1 bits m of u[b] (g_rows: k generator rows, bit c = parity column c; degree <= 32).
 * pl_crc_check:    valid[b] = 1 iff the parity of the whole received word[b] (len bits, g_rows: len
 *                  generator rows) is all zero, i.e. its last degree bits are the CRC of the first
 *                  len - degree bits; else 0.
 * pl_gather_rows:  out[b, j] = in[b, idx[j]], j < n_out <= 4096 (rate matching).
 * pl_rate_recover: out[b, j] = src_a[j] < 0 ? fill[j] : in[b, src_a[j]] (+ in[b, src_b[j]] if
 *                  src_b (nullable) has src_b[j] >= 0), j < n <= 2048 (de-interleaving, puncturing
 *                  = fill 0, shortening = fill -llr_max, repetition = the sum, sub-block
 *                  de-interleaving folded into one table). */
int pl_crc_attach(const float* u, int64_t bs, int32_t k, const uint32_t* g_rows, int32_t degree, float* out,
                  void* hip_stream);
int pl_crc_check(const float* word, int64_t bs, int32_t len, const uint32_t* g_rows, int32_t degree,
                 uint8_t* valid, void* hip_stream);
int pl_gather_rows(const float* in, int64_t bs, int32_t n_in, const int32_t* idx, int32_t n_out, float* out,
                   void* hip_stream);
int pl_rate_recover(const float* llr, int64_t bs, int32_t e, const int32_t* src_a, const int32_t* src_b,
                    const float* fill, int32_t n, float* out, void* hip_stream);

/* Monte-Carlo caller side, fused (polar_amd.channel.FusedAWGN, polar_amd.sim):
 * pl_awgn_qpsk_llr: System_AWGN_model.forward up to the decoder call (x_run_sn_polar/z_sys_model/
 *                  awgn_model.py:33-41) for rows row0 .. row0+bs-1 of a random stream: information bits
 *                  (BinarySource, my_sn/trans/binary_source.py:18-19; Philox4x32-10 keyed by seed,
 *                  counter (row, iteration)), codeword x = u G_n with the plan's frozen set
 *                  (x_run enc.py:30-43), Gray QPSK (mapping.py:136-149), AWGN of variance no
 *                  (awgn.py:19-29), logits log P(b=1)/P(b=0) (mapping.py:225-241).
 *                  u_out (nullable): [bs, k] fp32 0/1; llr_out: [bs, n] fp32.  no > 0.
 *                  Stream keys: row0 + row is the 64-bit counter row (words 0-1); iteration is
 *                  one 32-bit counter word, so 0 <= iteration < 2^32 (PL_EINVAL otherwise).
 *                  polar_amd.channel.FusedAWGN keys a draw by (SNR point, iteration) with the
 *                  point in the row's high word: row0 + (point << 32), iteration.
 * pl_count_errors: count_errors + count_block_errors (my_sn/sim.py:7-18) of two [rows, k] fp32 0/1
 *                  tensors: counts[0] += differing elements, counts[1] += rows with a difference
 *                  (int64 device counters, accumulated).
 * pl_awgn_qpsk_llr_bits: pl_awgn_qpsk_llr with the information bits packed instead of fp32:
 *                  ubits_out (nullable) [bs, ceil(k/32)] uint32, bit m % 32 of word m / 32 = bit m
 *                  (bits past k zero).  Same stream, same logits.
 * pl_sc_decode_count: SC decode (as pl_sc_decode) fused with the harness's error count: instead of
 *                  writing the decided bits, compares them with ref_bits (packed as above) and
 *                  accumulates counts[0] += bit errors, counts[1] += block errors (int64 device
 *                  counters) -- pl_sc_decode + pl_count_errors in one pass (sim.py:84-100).
 *                  workspace: pl_sc_count_workspace_size(plan, bs) bytes of device scratch.
 *                  PL_ENOTSUP for plans on the generic SC kernel (pl_plan_kernel: 0).
 * pl_sc_sim_count: one whole Monte-Carlo iteration of the harness (System_AWGN_model.forward,
 *                  awgn_model.py:33-44, then sim.py:84-100's counters) in the SC kernel itself:
 *                  information bits, polar encoding, QPSK, AWGN and logits are generated in the
 *                  decoder's lane layout (Philox4x32-10 keyed by seed, counter (row0 + row,
 *                  iteration, stream word); streams distinct from pl_awgn_qpsk_llr's), decoded, and
 *                  compared in registers: counts[0] += bit errors, counts[1] += block errors.  No
 *                  LLR or bit row is written unless llr_dump ([bs, n] fp32 logits) / u_dump ([bs, k]
 *                  fp32 information bits) are given (nullable; for tests).  workspace as
 *                  pl_sc_decode_count.  PL_ENOTSUP unless the plan's specialised kernel has 64
 *                  channel slots per lane (min-sum n = 64 ... 1024; pl_plan_kernel: 1).
 *                  0 <= iteration < 2^32, as pl_awgn_qpsk_llr. */
int pl_awgn_qpsk_llr(const pl_plan* plan, uint64_t seed, uint64_t iteration, int64_t row0, int64_t bs, float no,
                     float* u_out, float* llr_out, void* hip_stream);
int pl_awgn_qpsk_llr_bits(const pl_plan* plan, uint64_t seed, uint64_t iteration, int64_t row0, int64_t bs,
                          float no, uint32_t* ubits_out, float* llr_out, void* hip_stream);
int pl_count_errors(const float* a, const float* b, int64_t rows, int32_t k, int64_t* counts, void* hip_stream);
size_t pl_sc_count_workspace_size(const pl_plan* plan, int64_t bs);
int pl_sc_decode_count(const pl_plan* plan, const float* llr_logits, int64_t bs, const uint32_t* ref_bits,
                       int64_t* counts, void* workspace, size_t ws_bytes, void* hip_stream);
int pl_sc_sim_count(const pl_plan* plan, uint64_t seed, uint64_t iteration, int64_t row0, int64_t bs, float no,
                    int64_t* counts, void* workspace, size_t ws_bytes, float* llr_dump, float* u_dump,
                    void* hip_stream);

/* The 5G NR link, fused (polar_amd.channel.FusedAWGN5G):
 * pl_nr_awgn_qpsk_llr: for rows row0 .. row0+bs-1 of the keyed stream of pl_awgn_qpsk_llr, everything
 *                  from the information bits to the mother decoder's input in one launch: BinarySource,
 *                  Polar5GEncoder.forward (my_sn/fec/polar/enc.py:359-392), Gray QPSK, AWGN of variance
 *                  no, the demapper, and rate recovery (Polar5GDecoder.forward, dec.py:609-638).
 *                  plan: the mother code (32 <= n <= 1024, k = k_target + crc_degree).  The k_target
 *                  information bits of a row are those pl_awgn_qpsk_llr draws for a code with k_target
 *                  information bits (Philox domain 0).  g_rows / crc_degree: pl_crc_attach's tables and
 *                  bit order.  Transmitted bit e < E is c[rm_idx[e]] of the mother codeword c (rm_idx:
 *                  E entries, each < n); E even, 2 <= E <= 2176 (PL_EINVAL otherwise).  The noise of
 *                  positions 4c .. 4c+3 is Philox block c of domain 1 of the row; logit = -2 sqrt(2) y / no.
 *                  src_a / src_b (nullable) / fill (nullable): pl_rate_recover's tables (n entries,
 *                  indices < E) and arithmetic, one fp32 add where two copies combine.
 *                  Outputs (all nullable but llr_out): ubits_out [bs, ceil(k_target/32)] packed
 *                  information bits (bits past k_target zero), u_out [bs, k_target] fp32 0/1,
 *                  llr_ch_out [bs, E] fp32 channel logits (for tests), llr_out [bs, n] fp32 mother-code
 *                  logits.  no > 0, 0 <= iteration < 2^32 as pl_awgn_qpsk_llr; bs == 0 is PL_OK.
 * pl_count_errors_packed: bits [bs, row_len] decided bits of kind PL_OUT_F32 / PL_OUT_U8 (nonzero = 1)
 *                  against ref_bits [bs, ceil(k_cmp/32)] packed as above: counts[0] += differing bits
 *                  among the first k_cmp <= row_len columns of each row, counts[1] += rows with one
 *                  (int64 device counters, accumulated, as pl_count_errors). */
int pl_nr_awgn_qpsk_llr(const pl_plan* plan, int32_t k_target, const uint32_t* g_rows, int32_t crc_degree,
                        const int32_t* rm_idx, int32_t e, const int32_t* src_a, const int32_t* src_b,
                        const float* fill, uint64_t seed, uint64_t iteration, int64_t row0, int64_t bs, float no,
                        uint32_t* ubits_out, float* u_out, float* llr_ch_out, float* llr_out, void* hip_stream);
int pl_count_errors_packed(const void* bits, int32_t kind, int64_t bs, int32_t row_len, int32_t k_cmp,
                           const uint32_t* ref_bits, int64_t* counts, void* hip_stream);

/* Square QAM for the two fused producers (polar_amd.channel.FusedAWGN / FusedAWGN5G, num_bits_per_symbol):
 * pl_awgn_qam_llr: pl_awgn_qpsk_llr / pl_awgn_qpsk_llr_bits with 2^m-QAM, m = bits_per_symbol in {2, 4, 6, 8}.
 *                  Symbol s of a row carries code positions m s .. m s + m - 1, the first bit the most
 *                  significant of the label (Mapper, my_sn/trans/mapping.py:135-148); the real part is the
 *                  Gray PAM level of bits b[0::2], the imaginary part that of b[1::2], unit energy
 *                  (mapping.py:7-48).  Noise: Philox domain 1, block c of the row serves symbols 2c (components
 *                  x, y: re, im) and 2c + 1 (z, w).  Logits log P(b=1)/P(b=0) by the reference's formula
 *                  (mapping.py:225-241, :195-205), evaluated per axis (for Gray square QAM the sum over the
 *                  2^m points factors), max-subtracted, fp32 with the library exp / log.
 *                  m must divide the plan's n (so m = 6 is refused for every plain power-of-two code).
 *                  u_out [bs, k] fp32 and ubits_out [bs, ceil(k/32)] packed (both nullable; the layouts of
 *                  pl_awgn_qpsk_llr / _bits), y_out (nullable, for tests) [bs, n/m, 2] fp32 received symbols
 *                  (re, im), llr_out [bs, n] fp32.  The information bits are those of pl_awgn_qpsk_llr for the
 *                  same key: the modulation does not change which codeword is drawn.
 *                  m == 2 launches the QPSK kernel with the same arguments (bit-identical to pl_awgn_qpsk_llr
 *                  and pl_awgn_qpsk_llr_bits); y_out must be NULL there.
 *                  PL_EINVAL (the message names the argument): bits_per_symbol not in {2, 4, 6, 8}, y_out with
 *                  m == 2, n % m != 0, no <= 0, iteration >= 2^32, negative bs / row0, no llr_out.  bs == 0 is PL_OK.
 * pl_nr_awgn_qam_llr: pl_nr_awgn_qpsk_llr with 2^m-QAM as above on the E transmitted positions (symbol s =
 *                  positions m s .. m s + m - 1 after rate matching), plus y_out (nullable) [bs, E/m, 2].  E must
 *                  be a multiple of m, m <= E <= 2176 (an odd symbol count leaves the second half of the last
 *                  noise block unused).  llr_out is pl_rate_recover of llr_ch_out, bit for bit.  Every other
 *                  argument, check and output as pl_nr_awgn_qpsk_llr; m == 2 calls it (y_out NULL). */
int pl_awgn_qam_llr(const pl_plan* plan, int32_t bits_per_symbol, uint64_t seed, uint64_t iteration, int64_t row0,
                    int64_t bs, float no, float* u_out, uint32_t* ubits_out, float* y_out, float* llr_out,
                    void* hip_stream);
int pl_nr_awgn_qam_llr(const pl_plan* plan, int32_t bits_per_symbol, int32_t k_target, const uint32_t* g_rows,
                       int32_t crc_degree, const int32_t* rm_idx, int32_t e, const int32_t* src_a, const int32_t* src_b,
                       const float* fill, uint64_t seed, uint64_t iteration, int64_t row0, int64_t bs, float no,
                       uint32_t* ubits_out, float* u_out, float* y_out, float* llr_ch_out, float* llr_out,
                       void* hip_stream);

/* Ordered-statistics decoding (OSD) of a short binary linear code: OSDecoder, my_sn/fec/osd/dec.py
 * (polar_amd.OSDecoder).  Order-t OSD is the usual estimate of the maximum-likelihood curve of a short
 * code, the yardstick for a list decoder.  One wave decodes one codeword (csrc/osd_kernel.hip):
 *   1. clip the logits to +-100 and order the positions by |llr| descending -- among equal |llr| the
 *      lower index first (the reference's argsort leaves that order open);
 *   2. permute the columns of G into that order and eliminate, for row c = 0 .. k-1 in turn: the pivot
 *      is the first 1 of row c, row c is XORed into every other row with a 1 there (dec.py:107-147);
 *   3. hard-decide the k pivot positions (llr > 0 is 1) and re-encode them to c0;
 *   4. for order i = 1 .. t, every i-subset of the k basis rows in itertools.combinations order: the
 *      candidate is c0 XOR those rows, its metric mean_j log(1 + exp(llr_j (1 - 2 c_j))); the first
 *      minimum of an order wins, and replaces the incumbent only when strictly smaller.  The search
 *      compares the metric differences -sum_{j in supp e} llr_j (1 - 2 c0_j) in fp64, which needs no
 *      exp or log; a pattern's index counts the orders in turn, each in combinations order.
 * pl_osd_plan_create: gm is a HOST pointer to the k x n generator matrix, one byte per entry (nonzero
 *                  = 1), row-major: the encoder applied to the identity (dec.py:38-40).
 *                  Envelope: 1 <= k <= 128, k <= n <= 256, 0 <= t <= min(k, 4) and at most 2^22 patterns
 *                  (sum of C(k, i), i = 1 .. t: t = 3 at k = 128 and t = 4 at k = 64 fit, t = 4 at
 *                  k = 128 does not); PL_ENOTSUP outside it.  PL_EINVAL (the message names the argument)
 *                  for a NULL pointer, a negative size and a gm that is not of rank k (the reference
 *                  silently picks column 0 as the pivot of an all-zero row).  These checks run before
 *                  any HIP call.  The plan is bound to the device current at the call, like a pl_plan;
 *                  created where there is no GPU, it only answers pl_osd_plan_info.
 * pl_osd_plan_info: k, n, t and the number of patterns of the search (any pointer may be NULL).
 * pl_osd_decode:   llr_logits [bs, n] fp32 logits log P(1)/P(0).  out_cw [bs, n]: the decided codeword in
 *                  channel order, PL_OUT_F32 or PL_OUT_U8.  out_dist (nullable) [bs] fp64: the metric of
 *                  the returned word.  out_pattern (nullable) [bs] int32: -1 when c0 is returned, else the
 *                  index of the winning pattern.  No allocation per call; batches above 2^20 rows are
 *                  launched in chunks.  A stream of another device is PL_EINVAL; bs == 0 is PL_OK.  +-Inf
 *                  is clipped like any large value; NaN is not supported. */
typedef struct pl_osd_plan pl_osd_plan;
int pl_osd_plan_create(pl_osd_plan** out, int32_t k, int32_t n, const uint8_t* gm, int32_t t);
int pl_osd_plan_destroy(pl_osd_plan* plan);
int pl_osd_plan_info(const pl_osd_plan* plan, int32_t* k, int32_t* n, int32_t* t, int64_t* n_patterns);
int pl_osd_decode(const pl_osd_plan* plan, const float* llr_logits, int64_t bs, void* out_cw, int32_t out_kind,
                  double* out_dist, int32_t* out_pattern, void* hip_stream);

/* Genie-aided SC for frozen-set design (polar_amd.design; csrc/genie_kernel.hip): the leaf LLR of every
 * position when all earlier bits are fed back correctly.
 * llr_logits [bs, n] fp32 logits log P(1)/P(0) (negated inside, as pl_sc_decode).
 * u_bits [bs, ceil(n/32)] uint32: the u-domain word, ALL n positions (bit m%32 of word m/32 =
 * position m; frozen positions carry their value, normally 0).
 * counts (nullable) [n] int64 device counters, accumulated: counts[i] += rows where
 * HD(leaf[i]) != u[i], HD(x) = !(x > 0).
 * leaf_out (nullable) [bs, n] fp32: the leaf LLRs alpha_0 (positive favours 0).
 * The transform, in place on a[0..n) = -logits, S = log2 n: beta_0 = u; beta_s is beta_{s-1} with
 * b[p] ^= b[p + 2^(s-1)] for every p whose index bit s-1 is 0 (the encoder butterfly stopped after s
 * stages); for s = S down to 1, h = 2^(s-1), every p whose index bit s-1 is 0: x = a[p], y = a[p+h],
 * a[p] = f(x, y), a[p+h] = g(x, y, beta_{s-1}[p]), f and g those of pl_sc_decode (min-sum on inputs
 * clipped to +-llr_max, or the exact f of PL_F_EXACT, full-range form when llr_max > 43; g unclipped,
 * one rounding).  After stage 1, a is the leaf vector.  counts[] is a sum of integers: reproducible.
 * n a power of two, 2 <= n <= 2048; bs == 0 is PL_OK; PL_EINVAL (the message names the argument) for a
 * bad n or f_mode, a NULL llr_logits or u_bits with bs > 0, both outputs NULL, negative bs.  No plan:
 * the stream's device is the caller's business, as for pl_crc_attach.  No allocation per call. */
int pl_genie_count(int32_t n, int32_t f_mode, float llr_max, const float* llr_logits, const uint32_t* u_bits,
                   int64_t bs, int64_t* counts, float* leaf_out, void* hip_stream);

/* Iterative belief-propagation (BP) decoding with soft output (polar_amd.BP_Dec; csrc/bp_kernel.hip): the
 * "BP" decoder my_sn/fec/polar/dec.py names (its first line, and dec_type of Polar5GDecoder) and does not
 * contain.  The only decoder here that returns soft information.
 * plan: a list-size-1 plan; its n (2 <= n <= 1024), frozen set, f_mode and llr_max (lmax below) are used.
 * llr_logits [bs, n] fp32 logits log P(1)/P(0); inside, an LLR is a = -logit (positive favours 0).
 * Messages L[s][i] (towards u) and R[s][i] (towards the channel), s = 0 .. S = log2 n, on the encoder
 * butterfly: for s = 1 .. S, h = 2^(s-1), every p whose index bit s-1 is 0, one unit joins (s-1, p),
 * (s-1, p+h), (s, p), (s, p+h).  L[S][i] = clip(-logit[i]); R[0][i] = +lmax at frozen positions, 0 at
 * information positions; every other message starts at 0.  clip(v) = med3(v, -lmax, lmax).
 * f: PL_F_MINSUM: magnitude min(|x|, |y|, lmax) -- times scale, rounded to fp32 once, when scale < 1 --
 * with the xor of the two sign bits; PL_F_EXACT: pl_sc_decode's exact f (inputs clipped inside, the
 * full-range form when lmax > 43).
 * One iteration: the R pass, s = 1 .. S, every unit:
 *     R[s][p]   = clip(f(R[s-1][p], L[s][p+h] + R[s-1][p+h]))
 *     R[s][p+h] = clip(f(R[s-1][p], L[s][p]) + R[s-1][p+h])
 * then the L pass, s = S .. 1, every unit:
 *     L[s-1][p]   = clip(f(L[s][p], L[s][p+h] + R[s-1][p+h]))
 *     L[s-1][p+h] = clip(f(L[s][p], R[s-1][p]) + L[s][p+h])
 * every + one fp32 rounding, the inner sum not clipped before f.  A stage writes each message once and
 * reads only the neighbouring stage: the result does not depend on the schedule.
 * Outputs after the last iteration run (any may be NULL, not all):
 *   out_bits [bs, k], PL_OUT_F32 / PL_OUT_U8: !(L[0][i] > 0) at the information positions, ascending;
 *   soft_u [bs, k] fp32: -L[0][i] there, logits log P(1)/P(0) like the input;
 *   ext_x [bs, n] fp32: -R[S][i], the extrinsic logits of the code bits;
 *   iters [bs] int32: the iterations the row ran.
 * flags: 0 or PL_BP_EARLY_STOP: after each iteration, u^ = the hard decisions over all n positions (frozen
 * ones 0) and x^[i] = !(L[S][i] + R[S][i] > 0); a row whose u^ encodes to x^ stops and keeps the messages
 * of that iteration.  Without the flag, and for a row that never stops, iters is num_iter.
 * No allocation and no host synchronisation: the call can be captured into a HIP graph.  bs == 0 is PL_OK.
 * PL_EINVAL (the message names the argument): num_iter < 1, scale outside (0, 1], scale != 1 with
 * PL_F_EXACT, a list plan, all four outputs NULL, negative bs, a stream of another device.  PL_ENOTSUP:
 * n = 2048 (the messages of a codeword, (2 S + 1) n fp32, must fit one CU's LDS).  NaN and Inf inputs are
 * not supported. */
#define PL_BP_EARLY_STOP 1u
int pl_bp_decode(const pl_plan* plan, const float* llr_logits, int64_t bs, int32_t num_iter, float scale,
                 uint32_t flags, void* out_bits, int32_t out_kind, float* soft_u, float* ext_x, int32_t* iters,
                 void* hip_stream);

/* Soft-cancellation (SCAN) decoding with soft output (Fayyaz and Barry 2014; polar_amd.SCAN_Dec;
 * csrc/scan_kernel.hip).  The reference has no such decoder.  pl_bp_decode's factor graph, unit equations and
 * outputs on the schedule of the SC tree walk: decided and frozen leaves reach the rest of the tree within one
 * iteration, so 1 .. 4 iterations do what flooding BP needs tens for.
 * plan: a list-size-1 plan; its n (2 <= n <= 2048), frozen set, f_mode and llr_max (lmax below) are used.
 * llr_logits [bs, n] fp32 logits log P(1)/P(0); inside, an LLR is a = -logit (positive favours 0).
 * Messages L[s][i] (towards u) and R[s][i] (towards the channel), s = 0 .. S = log2 n.  L[S][i] =
 * clip(-logit[i]); R[0][i] = +lmax at frozen positions, 0 at information positions; every other message starts
 * at 0.  clip(v) = med3(v, -lmax, lmax).
 * f: PL_F_MINSUM: magnitude min(|x|, |y|, lmax) -- times scale, rounded to fp32 once, when scale < 1 --
 * with the xor of the two sign bits; PL_F_EXACT: pl_sc_decode's exact f (inputs clipped inside, the
 * full-range form when lmax > 43).
 * One iteration is node(S, 0).  node(0, .) does nothing.  node(s, b), s >= 1, h = 2^(s-1), for every i in
 * [b, b+h):
 *     L[s-1][i]   = clip(f(L[s][i], L[s][i+h] + R[s-1][i+h]))    R[s-1][i+h]: the previous iteration's value
 *     node(s-1, b)                                               (0 in the first)
 *     L[s-1][i+h] = clip(f(L[s][i], R[s-1][i]) + L[s][i+h])      R[s-1][i]: just written by the left child
 *     node(s-1, b+h)
 *     R[s][i]     = clip(f(R[s-1][i], L[s][i+h] + R[s-1][i+h]))
 *     R[s][i+h]   = clip(f(R[s-1][i], L[s][i]) + R[s-1][i+h])
 * every + one fp32 rounding, the inner sum not clipped before f.  These are pl_bp_decode's units.  Within a
 * node each message is written once: the values do not depend on how the i are spread over lanes.
 * Outputs after the last iteration run (any may be NULL, not all):
 *   out_bits [bs, k], PL_OUT_F32 / PL_OUT_U8: !(L[0][i] > 0) at the information positions, ascending;
 *   soft_u [bs, k] fp32: -L[0][i] there, logits log P(1)/P(0) like the input;
 *   ext_x [bs, n] fp32: -R[S][i], the extrinsic logits of the code bits;
 *   iters [bs] int32: the iterations the row ran.
 * flags: 0 or PL_SCAN_EARLY_STOP: after each iteration, u^ = the hard decisions over all n positions (frozen
 * ones 0) and x^[i] = !(L[S][i] + R[S][i] > 0); a row whose u^ encodes to x^ stops and keeps the messages
 * of that iteration.  Without the flag, and for a row that never stops, iters is num_iter.
 * No allocation, no workspace and no host synchronisation: the call can be captured into a HIP graph.  Natural
 * alignment only.  bs == 0 is PL_OK.  PL_EINVAL (the message names the argument): num_iter < 1, scale outside
 * (0, 1], scale != 1 with PL_F_EXACT, a list plan, all four outputs NULL, negative bs, a stream of another
 * device.  NaN and Inf inputs are not supported. */
#define PL_SCAN_EARLY_STOP 1u
int pl_scan_decode(const pl_plan* plan, const float* llr_logits, int64_t bs, int32_t num_iter, float scale,
                   uint32_t flags, void* out_bits, int32_t out_kind, float* soft_u, float* ext_x, int32_t* iters,
                   void* hip_stream);

/* CRC-aided successive-cancellation flip decoding (SC-Flip; Afisiadis, Balatsoukas-Stimming, Burg 2014;
 * polar_amd.SCF_Dec; csrc/scf_kernel.hip).  The reference has no such decoder.  SC first; a row whose SC
 * result fails the CRC is decoded again with its least reliable decision inverted, one bit per attempt.
 * plan: a list-size-1 plan (PL_EINVAL for a list plan) with a CRC (pl_plan_set_crc; PL_ENOTSUP without, as
 * pl_crc_status); its n, frozen set, f_mode, llr_max and SC kernel are used.  2 <= n <= 1024; n = 2048 is
 * PL_ENOTSUP.  llr_logits [bs, n] fp32 logits log P(1)/P(0); a = -logit.  f and g are pl_sc_decode's for the
 * plan, HD(x) = !(x > 0), frozen positions decide 0, a row "passes" iff pl_crc_status of its k bits is 1.
 * One row, T = max_flips (0 <= max_flips <= 64), T' = min(T, k):
 *   attempt 0: u^0 = the row pl_sc_decode returns for this plan, bit for bit (it is launched).  If it
 *     passes: out = u^0, crc_ok = 1, flip_pos = -1, attempts = 1.
 *   candidates: alpha_i = the fp32 LLR at leaf i on which attempt 0 decided position i -- what
 *     pl_genie_count's leaf_out[i] is when u_bits is u^0 over all n positions.  c_1 .. c_T' are the
 *     information positions in ascending (|alpha_i|, i) order: magnitudes compared as fp32 values, +0 and -0
 *     equal, the lower index first among equal magnitudes (min-sum gives many exact ties).
 *   attempt t = 1 .. T': SC from the same logits, leaf by leaf, with the attempt's own feedback, except that
 *     the decision at c_t is 1 - HD(alpha) of the attempt's own leaf LLR (which equals attempt 0's there).
 *     The smallest t that passes gives out, crc_ok = 1, flip_pos = c_t (a u-domain position, 0 .. n-1),
 *     attempts = 1 + t.  If none passes: out = u^0, crc_ok = 0, flip_pos = -1, attempts = 1 + T'.
 * attempts is the number of SC decodes the sequential algorithm runs; the kernel runs several attempts of a
 * row side by side and keeps the first that passes, which gives the same outputs.
 * max_flips = 0 is pl_sc_decode plus pl_crc_status (attempts = 1); values above k behave as k.
 * out_bits [bs, k], PL_OUT_F32 / PL_OUT_U8.  crc_ok [bs] bytes, flip_pos [bs] int32, attempts [bs] int32:
 * each nullable.
 * workspace: device scratch of pl_scf_workspace_size(plan, bs, max_flips) bytes, required: 5 bytes per row
 * for the CRC flags and the list of failing rows, sized for every row failing, and 4.25 KiB of counters.
 * No allocation per call and NO host synchronisation: the number of failing rows stays on the device, the
 * second stage runs a fixed grid that strides over it, and the call can be captured into a HIP graph.
 * bs == 0 is PL_OK.  PL_EINVAL (the message names the argument): a NULL or list plan, max_flips outside
 * [0, 64], bs negative or >= 2^31, an unknown out_kind, a NULL llr_logits or out_bits with bs > 0, a NULL or
 * short workspace, a stream of another device.  Every check but the last runs before any HIP call.
 * NaN inputs are not supported. */
size_t pl_scf_workspace_size(const pl_plan* plan, int64_t bs, int32_t max_flips);
int pl_scf_decode(const pl_plan* plan, const float* llr_logits, int64_t bs, int32_t max_flips, void* out_bits,
                  int32_t out_kind, uint8_t* crc_ok, int32_t* flip_pos, int32_t* attempts, void* workspace,
                  size_t ws_bytes, void* hip_stream);

/* Fixed-point successive-cancellation decoding on int8 LLRs, and the quantiser that produces them
 * (polar_amd.SCQ_Dec; csrc/scq_kernel.hip).  The reference has no such decoder: it answers how many LLR bits a
 * hardware SC decoder needs.  Everything is integer arithmetic, so the outputs equal the numpy restatement
 * tests/golden/scq_ref.py bit for bit on every input.
 * Cmax = 2^(q_channel-1) - 1, Imax = 2^(q_internal-1) - 1, 2 <= q_channel <= q_internal <= 8 (each function
 * checks the width it is given; the order between the two is the caller's to keep: the decoder clamps what it
 * loads to +-Imax either way).
 *
 * pl_llr_quantize: llr_logits [count] fp32 logits log P(1)/P(0) (pl_sc_decode's sign convention; the quantiser
 * does not negate, the decoder does), count a number of elements, so any row length is served.
 *   t = logit * inv_step (one fp32 rounding), q = rint(med3(t, -Cmax, Cmax)) with ties to even, stored as int8
 *   in out_q [count].  +-Inf saturates to +-Cmax; NaN is not supported.  count == 0 is PL_OK.
 * pl_scq_decode: plan is a list-size-1 plan of which only n and the frozen set are used (f_mode and llr_max are
 * ignored, and the specialised SC kernel is never involved), 2 <= n <= 2048.  llr_q [bs, n] int8, any value
 * including -128; 16-byte aligned when n >= 16 (the rows are read 16 LLRs at a time).  out_bits [bs, k],
 * PL_OUT_F32 / PL_OUT_U8, information positions ascending, as pl_sc_decode.
 *   load:  a_i = -clamp(llr_q_i, -Imax, Imax)            (positive favours 0, as in the float kernels)
 *   f(x, y) = sgn(x) sgn(y) min(|x|, |y|), sgn(0) = 0    (the range is symmetric: no overflow)
 *   g(x, y, b) = clamp(y + (1 - 2b) x, -Imax, Imax)
 *   leaf:  a frozen position decides 0, any other HD(a) = !(a > 0), so 0 decides 1 (polar_sc.py:94-97)
 *   partial sums and order: the plain SC recursion, the left child on f, the right child on g with the left
 *   child's re-encoded bits.
 * No allocation per call and no host synchronisation: both calls can be captured into a HIP graph.  bs == 0 is
 * PL_OK.  PL_EINVAL (the message names the argument): a NULL or list plan, q_channel or q_internal outside
 * [2, 8], a negative bs or count, an unknown out_kind, a NULL (or, for llr_q, misaligned) buffer with bs > 0 or
 * count > 0, an inv_step that is not positive and finite, a stream of another device than the plan's
 * (pl_llr_quantize has no plan: its stream and buffers are the caller's to keep on one device).  Every check but
 * the last runs before any HIP call. */
int pl_llr_quantize(const float* llr_logits, int64_t count, float inv_step, int32_t q_channel, int8_t* out_q,
                    void* hip_stream);
int pl_scq_decode(const pl_plan* plan, const int8_t* llr_q, int64_t bs, int32_t q_internal, void* out_bits,
                  int32_t out_kind, void* hip_stream);

/* Automorphism-ensemble SC decoding (AED; Geiselhart, Elkelesh, Ebada, Cammerer, ten Brink 2021;
 * polar_amd.AE_Dec; csrc/ae_kernel.hip).  The reference has no such decoder.  M permuted copies of the received
 * word are decoded by plain SC, the M candidate codewords are un-permuted, and the one closest to the received
 * word is kept.  It suits codes with a large automorphism group that SC is not invariant under: the
 * Reed-Muller codes the row-weight frozen sets are whenever k is a sum of binomials.
 * plan: a list-size-1 plan (PL_EINVAL for a list plan); its n, frozen set, f_mode and llr_max are used.
 * 2 <= n <= 1024; n = 2048 is PL_ENOTSUP.  llr_logits [bs, n] fp32 logits log P(1)/P(0).
 * perms: DEVICE memory, [num_perms][n] uint16, 1 <= num_perms <= 64; row t is a permutation pi_t of 0 .. n-1.
 * The call cannot check device data: the kernel masks every entry with n - 1, so a bad table never indexes
 * outside the row (the result is then unspecified, the accesses are not).
 * One row, a = -logits:
 *   candidate t: a'[i] = a[pi_t(i)].  a' is decoded by leaf-by-leaf SC exactly as an attempt of pl_scf_decode
 *     with no inverted decision: f of the plan, g = (1 - 2 u) x + y in one rounding, HD(x) = !(x > 0), nodes of
 *     nothing but frozen leaves decide 0, no repetition or parity-check shortcuts.  x' = the root's partial
 *     sums (the codeword SC decided on); the candidate codeword is x_t[pi_t(i)] = x'[i].
 *   metric: m_t = sum_i |a_i| [x_t[i] != HD(a_i)], accumulated in fp32; the order of the sum is not part of
 *     the contract.  Zero LLRs contribute nothing either way.
 *   winner: the t with the smallest fp32 metric as computed, the lowest t among equal fp32 values (the key
 *     (bits of m_t) << 32 | t compared as an unsigned integer; metrics are non-negative).
 * out_bits [bs, k], PL_OUT_F32 / PL_OUT_U8: (x_t* G_n) at the information positions.  best_idx [bs] int32 (t*)
 * and best_metric [bs] fp32 (m_t*): each nullable.  The output is defined for any permutation table: a pi_t
 * that is no automorphism of the code only makes a poor candidate.
 * No workspace, no allocation, NO host synchronisation: one launch on the caller's stream, capturable into a
 * HIP graph.  bs == 0 is PL_OK.  PL_EINVAL (the message names the argument): a NULL or list plan, num_perms
 * outside [1, 64], bs negative, an unknown out_kind, a NULL llr_logits, perms or out_bits with bs > 0, a
 * stream of another device.  Every check but the last runs before any HIP call.  NaN inputs are not supported. */
int pl_ae_decode(const pl_plan* plan, const float* llr_logits, int64_t bs, const uint16_t* perms, int32_t num_perms,
                 void* out_bits, int32_t out_kind, int32_t* best_idx, float* best_metric, void* hip_stream);

/* PAC codes (polarization-adjusted convolutional codes, Arikan 2019; polar_amd.PACEncoder, polar_amd.PAC_Dec;
 * csrc/pac_kernel.hip; restated in numpy by tests/golden/pac_ref.py, which the kernels equal value for value).
 * The reference has no PAC code.  A rate-1 convolutional precoder sits in front of the polar transform; the
 * frozen set is the rate profile (for the Reed-Muller profile: the row-weight sets of the reference).
 * Code.  plan: its n (a power of two, 2 <= n <= 1024) and frozen set (k information positions, ascending) are
 * used.  conv_mask: the generator (c_0, ..., c_m), bit j = c_j, c_0 = 1, 0 <= m <= 31.  The data word v has n
 * entries: the k data bits at the information positions, 0 elsewhere.  u_i = XOR_{j = 0..m} c_j v_{i-j}, v at a
 * negative index = 0; equivalently, with a 32-bit register r holding v_i at bit 0, v_{i-1} at bit 1, ...,
 * u_i = parity(r & conv_mask).  The codeword is x = u G_n, the transform and bit order of the plain encoder.
 * conv_mask = 1 is the plain polar code.
 * pl_pac_encode: data_bits [bs, k] fp32 (nonzero = 1) -> codewords [bs, n] fp32 0/1.
 * pl_pac_decode: a list decoder with the min-sum f, every value fp32.  llr_logits [bs, n] fp32 logits
 * log P(1)/P(0), negated inside: a positive LLR favours 0.  lmax = the plan's llr_max.
 *     f(x, y) = sign(x) sign(y) min(|x|, |y|, lmax);   g(x, y, b) = (b ? -x : x) + y, one fp32 add, not clipped.
 * Partial sums are built from u, not v.  Leaf i with LLR l, for each path: u0 = parity((r << 1) & conv_mask), the
 * precoder's output for v_i = 0; choosing v gives u = u0 ^ v; the path metric grows by |l| when u != (l < 0), by
 * 0 otherwise; r becomes (r << 1) | v.  A frozen leaf takes v = 0 -- its u is u0, which need not be 0.  An
 * information leaf makes 2L candidates, candidate c < L = (path c, v = 0), c >= L = (path c - L, v = 1); the L
 * smallest metrics survive, ordered by (metric, candidate index).  Path 0 starts at metric 0, the others at
 * +inf (inf + x = inf: the same order rule covers them).
 *   out_bits [bs, k], PL_OUT_F32 / PL_OUT_U8: the v bits of the lowest-metric path (the first minimum) at the
 *     information positions;
 *   out_pm [bs, list_size] fp32, may be NULL: the final metrics in ascending (metric, path) order.
 * list_size: a power of two in 1 ... 32, an argument of the call: the plan's own list_size is not used, the plan
 * supplies n, the frozen set and llr_max.  Every operation is an fp32 add, min, negate or compare.
 * No workspace, no allocation, no host synchronisation: one launch on the caller's stream, capturable into a
 * HIP graph.  Natural alignment only.  bs == 0 is PL_OK with no launch.
 * PL_EINVAL (the message names the argument): a NULL plan, conv_mask with bit 0 clear, list_size not a power of two
 * in 1 ... 32, bs negative, an unknown out_kind, a NULL data_bits / codewords / llr_logits / out_bits with bs > 0,
 * a stream of another device.  PL_ENOTSUP: a PL_F_EXACT plan, a plan with a CRC set, and an (n, list_size) whose
 * state, 4 (L n + n + 2 L max(n/32, 1) + 2 L) + L log2 n bytes, does not fit one work-group's LDS share of
 * 160 KiB: n <= 1024 (n = 1024 with list_size 32 fits); pl_pac_encode has the same bound on n.  NaN inputs are
 * not supported. */
int pl_pac_encode(const pl_plan* plan, uint32_t conv_mask, const float* data_bits, int64_t bs, float* codewords,
                  void* hip_stream);
int pl_pac_decode(const pl_plan* plan, uint32_t conv_mask, int32_t list_size, const float* llr_logits, int64_t bs,
                  void* out_bits, int32_t out_kind, float* out_pm, void* hip_stream);

/* Parity-constrained list decoding (polar_amd.PCL_Dec, polar_amd.dci; csrc/pcl_kernel.hip; restated in numpy by
 * tests/golden/pcl_ref.py, which the kernel equals value for value).  The reference has no such decoder.  A list
 * decoder in which a u-bit may be tied to earlier u-bits by an affine parity relation ("dynamic frozen bits"):
 * distributed CRC bits (38.212 downlink), parity-check polar codes, RM-polar codes with dynamic frozen bits;
 * pl_pac_decode is the special case of one convolution at every position.
 * Table.  pl_pcl_table_create(out, plan, C, pos, kind, rhs, mask): HOST arrays, validated on the host against the
 * plan's n and frozen set, uploaded to the plan's device (the current device must be the plan's).  C >= 0
 * constraints (the arrays may be NULL when C == 0):
 *   pos[C]    strictly ascending positions in [0, n), none frozen: a constrained position counts in k and
 *             appears in the output like any information position;
 *   kind[C]   PL_PCL_CHECK or PL_PCL_FORCE;
 *   rhs[C]    0 or 1;
 *   mask[C][W], W = max(n / 32, 1): bit (j & 31) of word j >> 5 = u-position j takes part; only non-frozen
 *             positions strictly below pos[c] may be set.
 * Constraint c states  u[pos[c]] = rhs[c] ^ parity(mask[c] & u).  Any violation is PL_EINVAL with a message that
 * names the constraint; a table never reaches a launch unvalidated.  pl_pcl_table_info: n, k of the plan it was made
 * for and C (any pointer may be NULL).  A table is immutable, device-bound and may be used from any stream.
 * pl_pcl_decode: the list decoder of pl_pac_decode with conv_mask = 1 -- min-sum f clipped at the plan's llr_max,
 * g one fp32 add, fp32 metrics, llr_logits [bs, n] fp32 log P(1)/P(0) negated inside, every leaf visited, path 0
 * starting at metric 0 and the others at +inf -- with these leaves:
 *   frozen leaf        u = 0; the metric grows by |l| when l < 0.
 *   information leaf   2L candidates, c < L = (path c, u = 0), c >= L = (path c - L, u = 1), each with the
 *                      parent's metric plus |l| where u != (l < 0); the first L by (metric, candidate index)
 *                      survive, +inf metrics included.
 *   FORCE leaf         no fork: path p takes u = rhs ^ parity(mask & u-decisions of p); its metric grows by |l|
 *                      where u != (l < 0).
 *   CHECK leaf         the fork and ranking of an information leaf; then every survivor whose own decisions give
 *                      u_pos ^ parity(mask & decisions) != rhs gets the metric +inf (it is dead, and loses every
 *                      later ranking against a live candidate).  If no path is alive after a CHECK leaf the row
 *                      stops at that leaf.
 * End: the first path of minimum metric is the output.
 *   out_bits [bs, k], PL_OUT_F32 / PL_OUT_U8: its u-bits at the plan's information positions, ascending,
 *     constrained positions included; a row with no path alive is all zero;
 *   out_pm [bs, list_size] fp32, may be NULL: the final metrics, ascending (metric, path); dead paths are +inf;
 *   out_ok [bs] bytes, may be NULL: 1 = a live path (finite metric) was output;
 *   out_stop [bs] int32, may be NULL: the leaf index at which the row stopped, n if it ran to the end.
 * list_size: a power of two in 1 ... 32, an argument of the call (the plan's own is not used).  No workspace, no
 * allocation, no host synchronisation: one launch on the caller's stream, capturable into a HIP graph.  Natural
 * alignment only.  bs == 0 is PL_OK with no launch.
 * PL_EINVAL (the message names the argument): a NULL plan or table, a table made for another n or frozen set or
 * on another device, list_size not a power of two in 1 ... 32, bs negative, an unknown out_kind, a NULL llr_logits
 * / out_bits with bs > 0, a stream of another device.  PL_ENOTSUP: a PL_F_EXACT plan, a plan with a CRC set, and an
 * (n, list_size) whose state, 4 (L n + n + 2 L max(n/32, 1) + 2 L) + L log2 n bytes, does not fit one
 * work-group's LDS share of 160 KiB: n <= 1024 (n = 1024 with list_size 32 fits); pl_pcl_table_create has the
 * same bound on n.  NaN inputs are not supported. */
#define PL_PCL_CHECK 0
#define PL_PCL_FORCE 1
typedef struct pl_pcl_table pl_pcl_table;
int pl_pcl_table_create(pl_pcl_table** out, const pl_plan* plan, int32_t num_constraints, const int32_t* pos,
                        const uint8_t* kind, const uint8_t* rhs, const uint32_t* mask);
int pl_pcl_table_destroy(pl_pcl_table* table);
int pl_pcl_table_info(const pl_pcl_table* table, int32_t* n, int32_t* k, int32_t* num_constraints);
int pl_pcl_decode(const pl_plan* plan, const pl_pcl_table* table, int32_t list_size, const float* llr_logits,
                  int64_t bs, void* out_bits, int32_t out_kind, float* out_pm, uint8_t* out_ok, int32_t* out_stop,
                  void* hip_stream);

/* pl_clock_probe: diagnostics, not on the reference's path.  One wave runs iters dependent VALU adds
 * and writes ticks[0] = s_memtime cycles (shader clock), ticks[1] = s_memrealtime ticks (100 MHz)
 * and ticks[2] (the chain's result) to the DEVICE buffer ticks[3]; clock GHz = 0.1 * ticks[0] /
 * ticks[1].  bench.py reads the clock around its timed region with it (DVFS moves the MI355X clock
 * with load and from box to box). */
int pl_clock_probe(uint64_t* ticks, int32_t iters, void* hip_stream);

const char* pl_last_error_string(void);
/* "polar_mi355x <version> (gfx950) src <16 hex digits>": the FNV-1a hash of the sources the library was
 * built from (polar_amd/build.py source_hash()). */
const char* pl_version(void);

#ifdef __cplusplus
}
#endif
#endif /* POLAR_MI355X_H */
