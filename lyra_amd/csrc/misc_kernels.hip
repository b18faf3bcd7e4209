// misc_kernels.hip -- residual vector quantizer, packet (un)packing, log-mel front end, state reset.
#include "kernels.h"
#include "lossy_plan.h"
#include "logmel_stages.h"
#include "resample_pass.h"
#include "cng_frame.h"

#ifdef LYRA_TIMING
extern "C" int lyra_hip_debug_timing_misc(long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lyra_tdbg), sizeof(long long) * 128);
}
#endif

namespace lyra {

#ifdef LYRA_PARKED
// The 64-term distance chain of one codeword, dims in ascending order: df = r - c, sq = df * df, sum = sum + sq, three
// separate fp32 operations per term as the graph's SUB / MUL / SUM (residual_vector_quantizer.cc:77-110 runs them
// through the `encode` subgraph).  `mine` = the lane's four residual dims; lane d4 of the row holds dims 4*d4..4*d4+3.
// x(lane L of the 16-lane row) - c: the row broadcast (DPP row_newbcast) rides on the subtraction's first operand, so the
// residual never travels through LDS and costs no instruction of its own.  (The compiler's DPP combiner does not fold a
// row_newbcast v_mov into its user, hence the instruction is spelled out; x must not have been written by the two
// preceding VALU instructions -- stage() separates the update of `mine` from the next chain.)
template <int L>
__device__ __forceinline__ float bcast_sub(float x, float c) {
  float d;
  asm("v_sub_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "=v"(d) : "v"(x), "v"(c), "n"(L));
  return d;
}
template <int D4>
__device__ __forceinline__ void rvq_terms(float& sum, float m0, float m1, float m2, float m3, const f32x4 (&row)[16]) {
  if constexpr (D4 < 16) {
    const f32x4 c = row[D4];
    const f32x4 df = {bcast_sub<D4>(m0, c[0]), bcast_sub<D4>(m1, c[1]), bcast_sub<D4>(m2, c[2]), bcast_sub<D4>(m3, c[3])};
    const f32x4 sq = df * df;
    sum = sum + sq[0];
    sum = sum + sq[1];
    sum = sum + sq[2];
    sum = sum + sq[3];
    rvq_terms<D4 + 1>(sum, m0, m1, m2, m3, row);
  }
}

// =============================================================================================
// RVQ encode, ALL-EXACT CHAIN FORM (rounds 1-3; since round 4 only in the variant build, for A/B and as the witness the
// shipped kernel is tested against, tests/test_gpu_side_kernels.py): quantizer.tflite `encode` (555 ops) + the bit-string
// assembly of ResidualVectorQuantizer::Quantize (lyra/residual_vector_quantizer.cc:77-110) + Packet<>::Pack
// (lyra/packet.h:91-122).  16 lanes = the 16 codewords of a stage; each lane runs the 64-term
// squared-distance sum in the oracle's order (separate multiply and add, d ascending), then a
// 16-lane DPP argmin with lowest-index tie break (ARG_MIN = first minimum).  4 frames per wavefront,
// 16 per workgroup.
//
// With 4096 frames there is exactly one 64-term chain per lane of the chip and one wavefront per SIMD: the kernel
// is a 46-step dependent chain and nothing but its own latency matters.  Per stage the critical path is
//   residual broadcast reads (LDS) -> 64 dependent adds -> 4 DPP steps -> winner row read (LDS) -> 3 ops -> LDS write,
// so everything that does not depend on the residual is taken off it:
//  * the lane's codeword row of stage k+1 (16 x ds_read_b128) is fetched into registers while stage k reduces and
//    updates (two register sets, the stage loop is unrolled by two);
//  * the residual lives in LDS (rs, row stride 68 floats so the four frames of a wavefront hit different banks),
//    shared by the 16 lanes of its frame with broadcast reads; lane j owns dims 4j..4j+3, keeps them in registers
//    and applies the graph's three fp32 ops r - (r + (q - r)) to them once per stage.  All 16 lanes of a frame sit
//    in one wavefront and LDS operations of a wavefront execute in order: the write-back needs no barrier;
//  * codebooks go global -> registers -> LDS in windows of W = 8 stages (rows padded to 68 floats: conflict-free
//    ds_read_b128 across the 16 code lanes), three buffers deep, one barrier per window: window w+1 is already in
//    LDS while window w computes (the cross-window prefetch needs it), window w+2 is in flight from L2.
// =============================================================================================
// W: stages per codebook window; PREFETCH: fetch the next stage's codeword row into a second register set while the
// current stage reduces (244 VGPRs) or read it at the start of its own stage (<= 128 VGPRs).
template <int W, bool PREFETCH>
__device__ __forceinline__ void rvq_encode_body(const float* __restrict__ cb, const float* __restrict__ feats, int B,
                                                int num_stages, int32_t* __restrict__ indices,
                                                uint8_t* __restrict__ packets, const int32_t* __restrict__ mask_ids,
                                                int32_t* __restrict__ packet_bytes) {
  constexpr int ROW = 68, WFLOATS = W * 16 * ROW;
  __shared__ __attribute__((aligned(16))) float cbs[3][WFLOATS];
  const int tid = threadIdx.x;
  const int j = tid & 15;
  const int frame = blockIdx.x * 16 + (tid >> 4);
  const int f = min(frame, B - 1);
  // DTX (lyra_encoder.cc:136-141): a stream whose hop is noise gets an empty packet; mask_ids[frame] < 0 marks it
  const bool live = frame < B && !(mask_ids && mask_ids[f] < 0);
  const int ldrow = tid >> 4, ldc4 = tid & 15;  // this thread's float4 of each stage's [16][64] codebook
  const f32x4 LYRA_GLOBAL* cbg = reinterpret_cast<const f32x4 LYRA_GLOBAL*>(as_global(cb)) + ldrow * 16 + ldc4;
  f32x4 stage_in[W];
  auto gload = [&](int win) {
#pragma unroll
    for (int v = 0; v < W; ++v) stage_in[v] = cbg[(size_t)min(win * W + v, 45) * 256];
  };   // (windows past the last stage re-read stage 45: never used, keeps the loop free of tail cases)
  auto lstore = [&](int win) {
    float* dst = cbs[win % 3] + ldrow * ROW + ldc4 * 4;
#pragma unroll
    for (int v = 0; v < W; ++v) *reinterpret_cast<f32x4*>(dst + v * 16 * ROW) = stage_in[v];
  };
  gload(0);
  f32x4 mine = *reinterpret_cast<const f32x4*>(&feats[(size_t)f * 64 + j * 4]);   // this lane's four residual dims
  lstore(0);
  gload(1);
  __syncthreads();
  const int nbytes = (num_stages + 1) >> 1;
  int cur = 0;
  f32x4 rowa[16], rowb[16];
  auto load_row = [&](f32x4 (&row)[16], int k) {
    const float* c = cbs[(k / W) % 3] + (k & (W - 1)) * 16 * ROW + j * ROW;
#pragma unroll
    for (int d4 = 0; d4 < 16; ++d4) row[d4] = *reinterpret_cast<const f32x4*>(&c[d4 * 4]);
  };
  if (PREFETCH) load_row(rowa, 0);
  auto stage = [&](int k, const f32x4 (&row)[16], f32x4 (&next)[16]) {
    const int u = k & (W - 1), win = k / W;
    if (u == 0) {
      // window win+1 -> LDS (fetched a window ago), request window win+2.  Buffer (win+1) % 3 last held window
      // win-2, which nobody reads any more: every wave passed the previous window's barrier, i.e. finished
      // window win-2, before any wave could get here.
      lstore(win + 1);
      gload(win + 2);
      __syncthreads();
    }
    if (!PREFETCH) load_row(next, k);   // (`row` and `next` are the same register set then)
    // residual dims 4*d4 .. 4*d4+3 live in lane d4 of the frame's 16-lane row: DPP row broadcast (row_newbcast, folded
    // into the subtraction's operand fetch) instead of a round trip through LDS
    float sum = 0.f;
    {
      float m0 = mine[0], m1 = mine[1], m2 = mine[2], m3 = mine[3];
      // a DPP operand must not have been written by the two preceding VALU instructions (`mine` is updated at the end
      // of the previous stage); tied to the data so it cannot be scheduled away from between the two
      asm volatile("s_nop 1" : "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3));
      rvq_terms<0>(sum, m0, m1, m2, m3, PREFETCH ? row : next);
    }
    // Off the critical path: issued after the chain and before the reduction, so the 16 reads drain while the DPP
    // steps run and the winner-row read below finds the LDS idle.
    __builtin_amdgcn_sched_barrier(0);
    if (PREFETCH && k + 1 < num_stages) load_row(next, k + 1);
    __builtin_amdgcn_sched_barrier(0);
    // ARG_MIN = first minimum, branch-free: the row minimum of the distance by a 16-lane all-reduce with DPP row
    // rotations (register-only, no LDS crossbar), then the lowest lane of the frame's 16-lane field that holds it
    // (ballot + find-first-set).  Distances are sums of squares (>= +0, finite for finite features).
    // (as unsigned integers: non-negative floats order like their bit patterns -- one v_min_u32 with a DPP operand per
    // step instead of move + two canonicalising maxima + minimum)
    unsigned mbits = __builtin_bit_cast(unsigned, sum);
#define LYRA_ROR_MINU(N) \
    asm("s_nop 1\n\tv_min_u32_dpp %0, %1, %1 row_ror:" #N " row_mask:0xf bank_mask:0xf" : "=v"(mbits) : "v"(mbits));
    LYRA_ROR_MINU(8) LYRA_ROR_MINU(4) LYRA_ROR_MINU(2) LYRA_ROR_MINU(1)
#undef LYRA_ROR_MINU
    const float m = __builtin_bit_cast(float, mbits);
    const unsigned long long holders = __builtin_amdgcn_ballot_w64(sum == m);
    const int best = __builtin_ctz((unsigned)(holders >> (tid & 48)) | 0x10000u) & 15;   // (& 15: NaN distances only)
    {  // r <- r - (r + (q - r)), the graph's three separate fp32 ops, on this lane's four dimensions
      const float* c = cbs[win % 3] + u * 16 * ROW;
      const f32x4 qv = *reinterpret_cast<const f32x4*>(&c[best * ROW + j * 4]);
      const f32x4 t1 = qv - mine;
      const f32x4 t2 = mine + t1;
      mine = mine - t2;
    }
    if (j == 0 && live) {
      if (indices) indices[(size_t)frame * 46 + k] = best;
      if (packets) {
        if (k & 1) packets[(size_t)frame * nbytes + (k >> 1)] = (uint8_t)(cur | best);
        else cur = best << 4;
      }
    }
  };
#pragma unroll 1
  for (int k = 0; k < num_stages; k += 2) {
    stage(k, rowa, PREFETCH ? rowb : rowa);
    if (k + 1 < num_stages) stage(k + 1, PREFETCH ? rowb : rowa, rowa);
  }
  if (j == 0 && frame < B && packet_bytes) packet_bytes[frame] = live ? nbytes : 0;
  if (j == 0 && live) {
    if (packets && (num_stages & 1)) packets[(size_t)frame * nbytes + (num_stages >> 1)] = (uint8_t)cur;
    if (indices)
      for (int k = num_stages; k < 46; ++k) indices[(size_t)frame * 46 + k] = -1;
  }
}

#endif   // LYRA_PARKED (chain form)

// =============================================================================================
// RVQ encode: replaces quantizer.tflite `encode` (555 ops) + the bit-string assembly of ResidualVectorQuantizer::Quantize
// (lyra/residual_vector_quantizer.cc:77-110) + Packet<>::Pack (lyra/packet.h:91-122).
// CERTIFIED SCREENING on the matrix pipe, the graph's exact chain only where the screen cannot decide.
//
// The reference's argmin is over S_k = the sequentially rounded fp32 sum above.  In exact arithmetic
// T_k = |r - c_k|^2 = |c_k|^2 - 2 r.c_k + |r|^2, and the 16 x 16 dot products of a stage's 16 codewords with 16 frames are
// ONE dense [16 x 64] x [64 x 16] GEMM: 16 v_mfma_f32_16x16x4_f32 per stage and wavefront instead of 4 x 192 dependent
// vector instructions per 4 frames.  A_k = N_k - 2 P_k (N_k = |c_k|^2 from the host, P_k the MFMA dot product) ranks the
// codewords up to a rounding error that is bounded rigorously (u = 2^-24, C = max_k |c_k| of the stage, any Rb >= |r|^2):
//     |S_k - T_k|           <= 67 u T_k                         (66 roundings on non-negative terms)
//     |A_k - (T_k - |r|^2)| <= 2 u |c_k|^2 + 142 u |r||c_k|     (N rounded once, <= 70 roundings on the dot product, one on A)
//     => S_j > S_k strictly whenever A_j - A_k > 280 u (|r| + C)^2, and (|r| + C)^2 <= 2 (Rb + C^2).
// The scores are compared as KEYS: bits(A_k + Rb + M) -- positive, so they order as integers -- with the low four bits
// replaced by k (a perturbation below 2^-19 of the score: one integer minimum yields winner AND index).  With the margin
//     M = 2^-14 (Rb + C^2)  >=  (560 u + 2^-16)(Rb + C^2)
// every codeword whose key exceeds the smallest key by more than M cannot be the reference's ARG_MIN.  If exactly one
// codeword is left it IS the reference's index -- certified, no exact sum computed.  Otherwise (near-ties, exact ties,
// NaNs: count != 1) the frame takes the exact chain -- the graph's three fp32 operations per term in ascending order, first
// minimum -- for all 16 codewords.  (On speech about one frame-stage in a thousand does: lyra_hip_debug_read(5).)
// Rb is carried from stage to stage: |r'|^2 <= T_winner + 7 u (..)^2 <= A_min + M + Rb + (error) => Rb' = (key_min + 2 M)(1 + 2^-10).
// The residual update r <- r - (r + (q - r)) is the graph's, bit for bit, so the residual the next stage sees -- and
// every index -- is the reference's.
//
// One wavefront = 16 frames = one MFMA N tile.  Lane (n = lane & 15, q = lane >> 4) owns dims 16 q .. 16 q + 15 of frame n
// (B operand of MFMA kk: dim 16 q + kk) and, as A operand, the same dims of codeword n -- both are plain 64-byte reads of
// the natural layouts, no repacking.  D[codeword 4 q + e][frame n]: a lane holds four codewords' scores of ONE frame, so
// the argmin is three minima in registers and a two-step all-reduce over the four 16-lane rows; the winner is then known
// to exactly the four lanes that hold the frame's residual.  Its dims come back from the A-fragment registers of lane
// (winner, q) by ds_bpermute: the codebook never passes through LDS or memory a second time, and the certified path has
// no barrier.
// =============================================================================================
// All-reduce over the four 16-lane rows of a wavefront, register to register: v_permlane16_swap (odd rows of the first
// operand <-> even rows of the second) pairs rows 0|1 and 2|3, v_permlane32_swap (upper half <-> lower half) pairs the halves.
__device__ __forceinline__ unsigned rows_min_u32(unsigned v) {
  const auto a = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  v = min(a[0], a[1]);
  const auto s = __builtin_amdgcn_permlane32_swap(v, v, false, false);   // [lo, lo], [hi, hi]
  return min(s[0], s[1]);
}
__device__ __forceinline__ unsigned rows_add_u32(unsigned v) {
  const auto a = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  v = a[0] + a[1];
  const auto s = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return s[0] + s[1];
}

__global__ __launch_bounds__(64) void rvq_encode_kernel(const float* __restrict__ cb, const float* __restrict__ cbn,
                                                        const float* __restrict__ feats, int B, int num_stages,
                                                        int32_t* __restrict__ indices, uint8_t* __restrict__ packets,
                                                        const int32_t* __restrict__ mask_ids,
                                                        int32_t* __restrict__ packet_bytes, unsigned* __restrict__ stats) {
  LYRA_STRESS(3);
  constexpr bool MIXED = false;
  const int32_t* const bits = nullptr;
  unsigned* const err = nullptr;
#include "rvq_encode_tile.inc"
}

__global__ __launch_bounds__(64) void rvq_encode_mixed_kernel(const float* __restrict__ cb, const float* __restrict__ cbn,
                                                              const float* __restrict__ feats, int B,
                                                              const int32_t* __restrict__ bits, uint8_t* __restrict__ packets,
                                                              const int32_t* __restrict__ mask_ids,
                                                              int32_t* __restrict__ packet_bytes, unsigned* __restrict__ stats,
                                                              unsigned* __restrict__ err) {
  LYRA_STRESS(3);
  constexpr bool MIXED = true;
  int num_stages = 0;              // the tile's bound, set from bits[]
  int32_t* const indices = nullptr;
#include "rvq_encode_tile.inc"
}

#ifdef LYRA_PARKED   // the all-exact chain kernels of rounds 2-3: bit-identical, kept for A/B in the variant build
// windows of two stages (26 KB of LDS), one register set (<= 128 VGPRs)
__global__ __launch_bounds__(256, 4) void rvq_encode_chain_kernel(const float* __restrict__ cb, const float* __restrict__ feats,
                                                            int B, int num_stages, int32_t* __restrict__ indices,
                                                            uint8_t* __restrict__ packets,
                                                            const int32_t* __restrict__ mask_ids,
                                                            int32_t* __restrict__ packet_bytes) {
  rvq_encode_body<2, false>(cb, feats, B, num_stages, indices, packets, mask_ids, packet_bytes);
}
// the 104 KB / 244-VGPR form
__global__ __launch_bounds__(256) void rvq_encode_wide_kernel(const float* __restrict__ cb, const float* __restrict__ feats,
                                                              int B, int num_stages, int32_t* __restrict__ indices,
                                                              uint8_t* __restrict__ packets,
                                                              const int32_t* __restrict__ mask_ids,
                                                              int32_t* __restrict__ packet_bytes) {
  rvq_encode_body<8, true>(cb, feats, B, num_stages, indices, packets, mask_ids, packet_bytes);
}
#endif

// RVQ decode: quantizer.tflite `decode` (233 ops) + the index extraction of DecodeToLossyFeatures
// (residual_vector_quantizer.cc:140-157).  ((v0 + v1) + v2) + ... strictly left to right, masked
// stages contribute v * 0.0f exactly as the graph does.
__global__ __launch_bounds__(256) void rvq_decode_kernel(const float* __restrict__ cb,
                                                          const int32_t* __restrict__ indices,
                                                          const uint8_t* __restrict__ packets, int num_stages, int B,
                                                          float* __restrict__ feats) {
  LYRA_STRESS(11);
  const int d = threadIdx.x & 63;
  const int frame = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (frame >= B) return;
  const int nbytes = (num_stages + 1) >> 1;
  float acc = 0.f;
#pragma unroll 2
  for (int k = 0; k < 46; ++k) {
    int id;
    if (packets) id = k < num_stages ? ((packets[(size_t)frame * nbytes + (k >> 1)] >> ((k & 1) ? 0 : 4)) & 15) : -1;
    else id = indices[(size_t)frame * 46 + k];
    float mask = id != -1 ? 1.f : 0.f;
    int i = id < 0 ? 0 : id;
    float v = cb[((size_t)k * 16 + i) * 64 + d] * mask;
    acc = k == 0 ? v : acc + v;
  }
  feats[(size_t)frame * 64 + d] = acc;
}

// The same for the packet rows of lyra_hip_decode_lossy_mixed_dev: MAX_PACKET_BYTES apart, each decoded at the
// stage count of its size (8 / 15 / 23 bytes: 16 / 30 / 46 stages, anything else 0 -- lossy_plan_mixed_kernel zeroes
// those rows' features).  bytes_from_bits: pkt_bytes holds bit counts, the size is (bits + 7) / 8 (mixed_bytes).
__global__ __launch_bounds__(256) void rvq_decode_mixed_kernel(const float* __restrict__ cb,
                                                                const uint8_t* __restrict__ packets,
                                                                const int32_t* __restrict__ pkt_bytes, int bytes_from_bits,
                                                                int B, float* __restrict__ feats) {
  LYRA_STRESS(11);
  const int d = threadIdx.x & 63;
  const int frame = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (frame >= B) return;
  const int pb = mixed_bytes(pkt_bytes[frame], bytes_from_bits);
  const int num_stages = pb == 8 ? 16 : pb == 15 ? 30 : pb == MAX_PACKET_BYTES ? 46 : 0;
  const uint8_t* row = packets + (size_t)frame * MAX_PACKET_BYTES;
  float acc = 0.f;
#pragma unroll 2
  for (int k = 0; k < 46; ++k) {
    const int id = k < num_stages ? ((row[k >> 1] >> ((k & 1) ? 0 : 4)) & 15) : -1;
    float mask = id != -1 ? 1.f : 0.f;
    int i = id < 0 ? 0 : id;
    float v = cb[((size_t)k * 16 + i) * 64 + d] * mask;
    acc = k == 0 ? v : acc + v;
  }
  feats[(size_t)frame * 64 + d] = acc;
}

// =============================================================================================
// log-mel: LogMelSpectrogramExtractorImpl::Extract (lyra/log_mel_spectrogram_extractor_impl.cc:96-126)
// as instantiated by NoiseEstimator (16 kHz, hop 320, window 640, 160 bands).
// One workgroup per PAIR of stream-frames: the two real windows are packed into one complex sequence
// (re = frame A, im = frame B), transformed by ONE fp64 FFT-1024 in five radix-4 passes in LDS (digit-reversed
// input, host-built twiddles), and separated again by the conjugate symmetry of real spectra -- a quarter of the
// butterfly passes per frame of a per-frame radix-2 transform.  Then |X|, one thread per mel band accumulating its
// bins in ascending order (== the reference's scatter loop order per band), log / floor.
// The spectrum differs from the oracle's radix-2 one in the last bits of the doubles; after the cast to float the
// two agree except when a band sum lies within ~1e-16 of a float rounding boundary.
// `state` / `stride` / `prev_off`: where the previous hop of each stream lives -- the plugin-level extractor's own
// region (R_MEL) or the slot of one of the two NoiseEstimators (R_NOISE_E / R_NOISE_D own their extractor).
// =============================================================================================
// NoiseEstimator::ReceiveSamples' decision + recurrence for one stream per wavefront (defined below, next to its notes)
// Everything noise_update_wave reads from a stream's slot, requested in ONE batch (noise_prefetch) ahead of the work
// whose result it is compared with: lane l of the stream's wavefront owns bins l, l + 64, l + 128.
struct NoisePre { float est[3], bound[3], sm[3], sq[3], tm[3]; int initialised, hops; };
__device__ __forceinline__ NoisePre noise_prefetch(int id, const uint8_t* state, bool mine);
template <int NW>
__device__ __forceinline__ void noise_update_wave(const NoiseP& P, int w, bool on, int id, int out_index, uint8_t* state,
                                                  const float* mel, const NoisePre& pre, float* sh, float* avg,
                                                  int32_t* is_noise_out, int32_t* masked_ids);

size_t logmel_lds_bytes() { return (size_t)1024 * 2 * 8; }             // the FFT buffer; everything later aliases dead parts of it
size_t cng_lds_bytes() { return (size_t)(1024 * 2 + 160) * 8; }      // (+160: the comfort-noise kernel's mel vector)

__device__ __forceinline__ int digit_reverse4_1024(int n) {   // reverse the five base-4 digits of n
  unsigned r = __brev((unsigned)n) >> 22;
  return (int)(((r & 0x2AAu) >> 1) | ((r & 0x155u) << 1));
}

// noise_tail != 0: `state` is a NoiseEstimator region and the kernel goes on with NoiseEstimator::ReceiveSamples' second
// half (noise_update_wave; wavefront f handles frame f) on the mel vector while it is still in LDS -- one launch and no
// trip of the 160 bins through HBM (`mel` may then be null).
// kMasked (logmel_masked_kernel): an id of -1 masks its row -- no history, no estimator, no output is touched (the decoder-
// side estimator of lyra_hip_decode_lossy_dev runs only on the received rows of a tick).
// kRates (logmel_rates_kernel): `Pp` is the array of the four rates' MelP (model.h d_mel_rate), `rates` holds one rate per
// row and `np_tab` the four NoiseP; the two streams of a workgroup may differ in rate, so the mel weights (a second table
// in LDS behind the FFT buffer), the band edges and the estimator's constants are selected per stream.
// kRowDtx (logmel_streams_kernel, with kRates): `dtx` holds one flag per row; a row with dtx[b] == 0 takes the path of an
// id -1 row (its estimator slot, the log-mel history included, is neither read nor written), except that masked_ids[b] is
// its id and is_noise_out[b] is 0.
size_t logmel_rates_lds_bytes() { return (size_t)(1024 * 2 + 514) * 8; }

template <bool kMasked, bool kRates = false, bool kRowDtx = false>
__device__ __forceinline__ void logmel_body(const MelP* __restrict__ Pp, const int16_t* __restrict__ pcm,
                                            const int32_t* __restrict__ ids, int B,
                                            uint8_t* __restrict__ state, int stride, int prev_off,
                                            float* __restrict__ mel, int noise_tail, NoiseP NP,
                                            int32_t* __restrict__ is_noise_out,
                                            int32_t* __restrict__ masked_ids,
                                            const int32_t* __restrict__ rates = nullptr,
                                            const NoiseP* __restrict__ np_tab = nullptr,
                                            const int32_t* __restrict__ dtx = nullptr) {
  const MelP& P = Pp[kRates ? 1 : 0];   // (window and twiddles are the same tables at every rate)
  extern __shared__ __attribute__((aligned(16))) double dsm[];
  // LDS (logmel_stages.h): the FFT buffer, then in its dead upper half the mel weights, the hop's mel vectors [2][160] floats
  // and noise_update_wave's [2][2][160] + [2][2] floats -- 16 KB per workgroup in all
  float* mel_lds = reinterpret_cast<float*>(dsm + LOGMEL_MEL);
  float* tail_sh = reinterpret_cast<float*>(dsm + LOGMEL_MEL + 160);
  float* tail_avg = reinterpret_cast<float*>(dsm + LOGMEL_MEL + 160 + 320);
  const int tid = threadIdx.x;
  int b0_ = blockIdx.x * 2;
  bool two_ = b0_ + 1 < B;
  if constexpr (kMasked) {   // a masked first row hands its place to the second one (out_index follows b0)
    if constexpr (kRates) {   // the list the extractor and the quantizer run on names masked rows too
      if (masked_ids && tid < 2 && b0_ + tid < B && ids[b0_ + tid] < 0) masked_ids[b0_ + tid] = -1;
    }
    bool ok0 = ids[b0_] >= 0, ok1 = two_ && ids[b0_ + 1] >= 0;
    if constexpr (kRowDtx) {   // a row whose encoder has no estimator: its id passes through, it is never noise, and from
      // here on it is an absent row -- decided before the first barrier, like the id -1 rows
      if (tid < 2 && b0_ + tid < B && ids[b0_ + tid] >= 0 && dtx[b0_ + tid] == 0) {
        if (masked_ids) masked_ids[b0_ + tid] = ids[b0_ + tid];
        if (is_noise_out) is_noise_out[b0_ + tid] = 0;
      }
      ok0 = ok0 && dtx[b0_] != 0;
      ok1 = ok1 && dtx[b0_ + 1] != 0;
    }
    if (!ok0 && !ok1) return;   // (workgroup-uniform, before any barrier)
    if (!ok0) b0_ += 1;
    two_ = ok0 && ok1;
  }
  const int b0 = b0_, b1 = b0 + 1;
  const bool two = two_;
  int ri0 = 1, ri1 = 1;
  if constexpr (kRates) { ri0 = mel_rate_index(rates[b0]); ri1 = mel_rate_index(rates[two ? b1 : b0]); }
  const MelP& PA = Pp[kRates ? ri0 : 0];   // frame 0's / frame 1's filterbank
  const MelP& PB = Pp[kRates ? ri1 : 0];
  LYRA_TSTAMP(110);
  int16_t* prev0 = reinterpret_cast<int16_t*>(state + (size_t)ids[b0] * stride + prev_off);
  int16_t* prev1 = reinterpret_cast<int16_t*>(state + (size_t)ids[two ? b1 : b0] * stride + prev_off);
  const int16_t* cur0 = pcm + (size_t)b0 * 320;
  const int16_t* cur1 = pcm + (size_t)(two ? b1 : b0) * 320;
  const LogmelWin win = logmel_window<kRates>(P, PA, PB, two, prev0, prev1, cur0, cur1, reinterpret_cast<f64x2*>(dsm), tid);
  __syncthreads();
  // every read of the old history is done: the hop becomes the history
  if (tid >= 64) { prev0[tid - 64] = win.b0s; if (two) prev1[tid - 64] = win.b1s; }
  if (tid < 128) { prev0[tid + 192] = win.c0s; if (two) prev1[tid + 192] = win.c1s; }
  LYRA_TSTAMP(111);
  logmel_fft<kRates>(P, win, dsm, tid);
  LYRA_TSTAMP(114);
  // the noise tail's view of the stream's slot is requested here, one batch, and arrives under the band sums
  const int tw = tid >> 6;
  const int tail_id = ids[(tw == 1 && two) ? b1 : b0];
  NoisePre npre = {};
  if (noise_tail) npre = noise_prefetch(tail_id, state, tw < 2);
  // (what a band item sums over is chosen per item under kRates: each frame has its own edges and weights)
  auto band_item = [&](int f, int band, int e0, int e1, int e2) {
    const float lm = logmel_band(dsm, f, e0, e1, e2, logmel_wl<kRates>(dsm, f));
    if (mel) mel[(size_t)(b0 + f) * 160 + band] = lm;
    if (noise_tail) mel_lds[f * 160 + band] = lm;
  };
  if (tid < 160) band_item(0, tid, win.be0, win.be1, win.be2);
  else if (two) band_item(1, tid - 96, win.be0, win.be1, win.be2);
  if (tid < 64 && two) band_item(1, tid, win.ce0, win.ce1, win.ce2);
  LYRA_TSTAMP(115);
  if (noise_tail) {   // (uniform)
    __syncthreads();
    LYRA_TSTAMP2(120);
    const int w = tw;
    const bool on = w == 0 || (w == 1 && two);
    if constexpr (kRates) NP = np_tab[(w & 1) ? ri1 : ri0];   // (wave-uniform)
    noise_update_wave<2>(NP, w, on, tail_id, b0 + (w & 1), state, mel_lds + (w & 1) * 160, npre, tail_sh, tail_avg,
                         is_noise_out, masked_ids);
  }
  LYRA_TSTAMP(119);
}

__global__ __launch_bounds__(256) void logmel_kernel(const MelP* __restrict__ Pp, const int16_t* __restrict__ pcm,
                                                      const int32_t* __restrict__ ids, int B,
                                                      uint8_t* __restrict__ state, int stride, int prev_off,
                                                      float* __restrict__ mel, int noise_tail, NoiseP NP,
                                                      int32_t* __restrict__ is_noise_out,
                                                      int32_t* __restrict__ masked_ids) {
  LYRA_STRESS(7);
  logmel_body<false>(Pp, pcm, ids, B, state, stride, prev_off, mel, noise_tail, NP, is_noise_out, masked_ids);
}
__global__ __launch_bounds__(256) void logmel_masked_kernel(const MelP* __restrict__ Pp, const int16_t* __restrict__ pcm,
                                                             const int32_t* __restrict__ ids, int B,
                                                             uint8_t* __restrict__ state, int stride, int prev_off,
                                                             float* __restrict__ mel, int noise_tail, NoiseP NP,
                                                             int32_t* __restrict__ is_noise_out,
                                                             int32_t* __restrict__ masked_ids) {
  LYRA_STRESS(7);
  logmel_body<true>(Pp, pcm, ids, B, state, stride, prev_off, mel, noise_tail, NP, is_noise_out, masked_ids);
}
// Per-stream sample rates (lyra_hip_encode_rates_dev): the DTX encoder's NoiseEstimator with each row's own filterbank
// and constants; rows of id -1 (invalid rate) are skipped as in logmel_masked_kernel and named -1 in masked_ids.
__global__ __launch_bounds__(256) void logmel_rates_kernel(const MelP* __restrict__ P4, const int16_t* __restrict__ pcm,
                                                            const int32_t* __restrict__ ids,
                                                            const int32_t* __restrict__ rates, int B,
                                                            uint8_t* __restrict__ state, int stride, int prev_off,
                                                            const NoiseP* __restrict__ np_tab,
                                                            int32_t* __restrict__ is_noise_out,
                                                            int32_t* __restrict__ masked_ids) {
  LYRA_STRESS(7);
  logmel_body<true, true>(P4, pcm, ids, B, state, stride, prev_off, nullptr, 1, NoiseP{}, is_noise_out, masked_ids, rates,
                          np_tab);
}

// Encoders with and without DTX in one batch (lyra_hip_encode_streams_dev): logmel_rates_kernel with one flag per row.  The
// reference creates no estimator for an encoder without DTX (lyra_encoder.cc:80): such a row's slot is not touched.
__global__ __launch_bounds__(256) void logmel_streams_kernel(const MelP* __restrict__ P4, const int16_t* __restrict__ pcm,
                                                              const int32_t* __restrict__ ids,
                                                              const int32_t* __restrict__ rates,
                                                              const int32_t* __restrict__ dtx, int B,
                                                              uint8_t* __restrict__ state, int stride, int prev_off,
                                                              const NoiseP* __restrict__ np_tab,
                                                              int32_t* __restrict__ is_noise_out,
                                                              int32_t* __restrict__ masked_ids) {
  LYRA_STRESS(7);
  logmel_body<true, true, true>(P4, pcm, ids, B, state, stride, prev_off, nullptr, 1, NoiseP{}, is_noise_out, masked_ids, rates,
                                np_tab, dtx);
}

// =============================================================================================
// NoiseEstimator::ReceiveSamples after the log-mel (lyra/noise_estimator.cc:161-173): ComputeIsNoise, then
// DecayBounds or UpdateNoiseEstimate (SmoothingFactor, UpdateMinAndTemp, ComputeBounds), for one hop of B streams.
// One wavefront per stream, lane l owns bins l, l + 64, l + 128 (< 160).  Same float operations in the same order
// as the reference; the two Average() sums are sequential (std::accumulate from 0.f) and run on one lane out of
// LDS.  std::exp(float) is evaluated as float(exp(double)): a <= 1 ULP double result rounds to the correctly rounded
// float, which is what the host libm returns.  masked_ids (optional): ids[i], or -1 where the hop is noise -- the
// stream list the DTX-enabled encoder runs on (lyra_encoder.cc:131-141).  (expf_via_double: kernels.h, shared with
// span_noise_scan_kernel.)
// =============================================================================================
// One wavefront = one stream (slot w of the workgroup, NW slots); every thread of the workgroup calls this (two
// workgroup barriers inside).  `mel`: the hop's 160 log-mel bins (LDS or global); `on`: the slot holds a real stream.
__device__ __forceinline__ NoisePre noise_prefetch(int id, const uint8_t* state, bool mine) {
  const int lane = threadIdx.x & 63;
  const uint8_t* base = state + (size_t)id * st::NOISE_BYTES;
  const int* hdr = reinterpret_cast<const int*>(base);
  NoisePre p;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int bin = lane + 64 * i;
    const bool ld = mine && bin < 160;
    p.est[i] = ld ? reinterpret_cast<const float*>(base + st::N_EST)[bin] : 0.f;
    p.bound[i] = ld ? reinterpret_cast<const float*>(base + st::N_BOUND)[bin] : 0.f;
    p.sm[i] = ld ? reinterpret_cast<const float*>(base + st::N_SMOOTH)[bin] : 0.f;
    p.sq[i] = ld ? reinterpret_cast<const float*>(base + st::N_SQ)[bin] : 0.f;
    p.tm[i] = ld ? reinterpret_cast<const float*>(base + st::N_TMPMIN)[bin] : 0.f;
  }
  p.initialised = hdr[st::N_INIT / 4];
  p.hops = hdr[st::N_HOPS / 4];
  return p;
}

template <int NW>
__device__ __forceinline__ void noise_update_wave(const NoiseP& P, int w, bool on, int id, int out_index, uint8_t* state,
                                                  const float* mel, const NoisePre& pre, float* sh, float* avg,
                                                  int32_t* is_noise_out, int32_t* masked_ids) {
  // sh: [NW][2][160] floats, avg: [NW][2] floats of LDS scratch owned by the caller
  const int lane = threadIdx.x & 63;
  const bool mine = w < NW;          // waves beyond the NW slots only take part in the barriers
  const int ws = mine ? w : 0;
  uint8_t* base = state + (size_t)id * st::NOISE_BYTES;
  int* hdr = reinterpret_cast<int*>(base);
  float* f_smooth = reinterpret_cast<float*>(base + st::N_SMOOTH);
  float* f_sq = reinterpret_cast<float*>(base + st::N_SQ);
  float* f_tmp = reinterpret_cast<float*>(base + st::N_TMPMIN);
  float* f_est = reinterpret_cast<float*>(base + st::N_EST);
  float* f_bound = reinterpret_cast<float*>(base + st::N_BOUND);
  float cur[3], est[3], bound[3];
  bool differs = false;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int bin = lane + 64 * i;
    cur[i] = est[i] = bound[i] = 0.f;
    if (bin < 160 && mine) {
      cur[i] = mel[bin];
      est[i] = pre.est[i];
      bound[i] = pre.bound[i];
      differs = differs || (__builtin_fabsf(cur[i] - est[i]) > bound[i]);
    }
  }
  const bool is_noise = __builtin_amdgcn_ballot_w64(differs) == 0ull;   // ComputeIsNoise (wave-uniform)
  const int initialised = pre.initialised;
  const int hops = pre.hops;
  float sm[3], sq[3], tm[3];
  if (!is_noise && mine) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int bin = lane + 64 * i;
      sm[i] = sq[i] = tm[i] = 0.f;
      if (bin < 160) {
        if (initialised) { sm[i] = pre.sm[i]; sq[i] = pre.sq[i]; tm[i] = pre.tm[i]; }
        else { sm[i] = cur[i]; sq[i] = cur[i] * cur[i]; tm[i] = cur[i]; }   // first update (noise_estimator.cc:180-186)
        sh[(ws * 2 + 0) * 160 + bin] = sm[i];
        sh[(ws * 2 + 1) * 160 + bin] = cur[i];
      }
    }
  }
  if (NW == 2) LYRA_TSTAMP2(116);
  __syncthreads();
  // Average(): sequential float sum from 0.f, then / 160 -- one lane per sum.  In a workgroup with a wavefront to spare
  // (256 threads, NW < 4) that wavefront does all 2 * NW sums at once (of rows a noise hop left unwritten too: unused),
  // off the path of the wavefronts that carry the streams.
  constexpr bool kSpare = NW < 4;
  // the per-bin factor of SmoothingFactor() does not need the averages: evaluated here, beside the summing lanes
  float ebin[3] = {0.f, 0.f, 0.f};
  if (!is_noise && mine) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float de = (sm[i] - est[i]) / 0.3f;
      ebin[i] = expf_via_double(-(de * de));
    }
  }
  if (kSpare ? (w == NW && lane < 2 * NW) : (!is_noise && mine && lane < 2)) {
    const int row = kSpare ? lane : ws * 2 + lane;
    float a = 0.f;
    for (int i = 0; i < 160; ++i) a = a + sh[row * 160 + i];
    avg[row] = a / 160.f;
  }
  __syncthreads();
  if (NW == 2) LYRA_TSTAMP2(117);
  if (!on || !mine) return;
  if (is_noise) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int bin = lane + 64 * i;
      if (bin < 160) f_bound[bin] = bound[i] * P.bound_decay;   // DecayBounds
    }
  } else {
    const float kPowDiff = 0.3f;
    const float dd = (avg[ws * 2 + 0] - avg[ws * 2 + 1]) / kPowDiff;
    const float correction = expf_via_double(-(dd * dd));
    const double logn = 5.075173815233827;   // std::log(160) in double (noise_bound_.size())
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int bin = lane + 64 * i;
      if (bin < 160) {
        const float sf = P.max_smoothing * correction * ebin[i];
        const float c2 = cur[i] * cur[i];
        const float nsm = sf * sm[i] + (1.f - sf) * cur[i];   // (-ffp-contract=off: every product rounded)
        const float nsq = sf * sq[i] + (1.f - sf) * c2;
        float nest, ntm;
        if (hops == 0) { nest = __builtin_fminf(tm[i], nsm); ntm = nsm; }                      // UpdateMinAndTemp
        else { nest = __builtin_fminf(est[i], nsm); ntm = __builtin_fminf(tm[i], nsm); }
        float var = nsq - nsm * nsm;
        var = var > 0.f ? var : 0.f;
        f_smooth[bin] = nsm; f_sq[bin] = nsq; f_tmp[bin] = ntm; f_est[bin] = nest;
        f_bound[bin] = (float)((double)0.9f * __builtin_sqrt((double)var * logn));            // ComputeBounds
      }
    }
  }
  if (NW == 2) LYRA_TSTAMP2(118);
  if (lane == 0) {
    if (!is_noise) {
      hdr[st::N_INIT / 4] = 1;
      hdr[st::N_HOPS / 4] = (hops + 1) % P.hops_per_update;
    }
    hdr[st::N_IS_NOISE / 4] = is_noise ? 1 : 0;
    if (is_noise_out) is_noise_out[out_index] = is_noise ? 1 : 0;
    if (masked_ids) masked_ids[out_index] = is_noise ? -1 : id;
  }
}

// Stand-alone form (mel computed elsewhere): four streams per workgroup.
__global__ __launch_bounds__(256) void noise_update_kernel(NoiseP P, const int32_t* __restrict__ ids, int B,
                                                            uint8_t* __restrict__ state, const float* __restrict__ mel,
                                                            int32_t* __restrict__ is_noise_out,
                                                            int32_t* __restrict__ masked_ids) {
  LYRA_STRESS(7);
  const int w = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + w;
  const bool on = b < B;
  const int bb = on ? b : B - 1;
  const int id = ids[bb];
  __shared__ float sh[4 * 2 * 160];
  __shared__ float avg[4 * 2];
  const NoisePre pre = noise_prefetch(id, state, true);
  noise_update_wave<4>(P, w, on, id, b, state, mel + (size_t)bb * 160, pre, sh, avg, is_noise_out, masked_ids);
}

// noise_estimate() / noise_bound() of B streams -> dense [B][160] (NoiseEstimator::noise_estimate, :229-231)
__global__ __launch_bounds__(256) void noise_read_kernel(const int32_t* __restrict__ ids, int B,
                                                          const uint8_t* __restrict__ state, int field_off,
                                                          float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * 160) return;
  const int b = i / 160, bin = i - b * 160;
  out[i] = reinterpret_cast<const float*>(state + (size_t)ids[b] * st::NOISE_BYTES + field_off)[bin];
}

// =============================================================================================
// Resampler::Resample (lyra/resampler.cc:57-62): audio_dsp::QResampler<float> restated as a polyphase FIR sampled from
// a Kaiser-windowed sinc (oracle/lyra_oracle.c lo_resampler_design builds the same table; parity statement there).
// One wavefront per stream, four streams per workgroup: [34 history samples | n_in new samples] as floats in LDS, taps
// oldest first in float with separately rounded products -- bitwise the oracle's loop.  up-sampling: `up` outputs per
// input sample; down-sampling: one output per `down` inputs, phase carried in the stream's slot.
// =============================================================================================
int resample_streams_per_wg() { return 4; }
size_t resample_lds_bytes(int n_in) { return (size_t)4 * ((st::RS_TAPS - 1 + n_in + 3) & ~3) * 4; }

__global__ __launch_bounds__(256) void resample_kernel(ResampleP P, const int32_t* __restrict__ ids, int B,
                                                        uint8_t* __restrict__ state, const int16_t* __restrict__ in,
                                                        int n_in, int in_stride, int16_t* __restrict__ out, int n_out,
                                                        int out_stride) {
  LYRA_STRESS(8);
  extern __shared__ __attribute__((aligned(16))) float rsb_all[];   // [4][RS_TAPS - 1 + n_in, padded to 4]
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x * 4 + w;
  const bool on = b < B;
  const int bb = on ? b : B - 1;
  const bool vec = ((in_stride | n_in) & 7) == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0;   // 16-byte items where the rows allow
  rs_stream_pass<true>(&P, rsb_all + w * ((RS_H + n_in + 3) & ~3), lane, state, ids[bb],
                       in + (size_t)bb * in_stride, n_in, vec, out + (size_t)b * out_stride, n_out, on);
}

// Per-stream sample rates (lyra_hip_encode_rates_dev / lyra_hip_decode_lossy_rates_dev): row b is resampled between
// rates[b] and 16 kHz with the design of its own rate.  tab = [2][3] designs, [dir][8000, 32000, 48000]; dir 0: rates[b]
// -> 16 kHz (rows hold rates[b] / 50 samples in, 320 out), dir 1: 16 kHz -> rates[b].  One wavefront per stream as above,
// so the design index is wave-uniform (readfirstlane) and the coefficients stay scalar operands; the LDS row is sized for
// 48 kHz.  A row at 16000 is copied through and its slot not touched; any other value that is not a codec rate writes
// nothing, is counted in *err and named -1 in ids_out (optional: ids[b] for every other row).  No workgroup barrier: a
// wavefront only reads the LDS row it wrote.
size_t resample_rates_lds_bytes() { return (size_t)4 * ((st::RS_TAPS - 1 + 960 + 3) & ~3) * 4; }

__global__ __launch_bounds__(256) void resample_rates_kernel(const ResampleP* __restrict__ tab, int dir,
                                                              const int32_t* __restrict__ rates,
                                                              const int32_t* __restrict__ ids, int B,
                                                              uint8_t* __restrict__ state, const int16_t* __restrict__ in,
                                                              int in_stride, int16_t* __restrict__ out, int out_stride,
                                                              int32_t* __restrict__ ids_out, unsigned* __restrict__ err) {
  LYRA_STRESS(8);
  extern __shared__ __attribute__((aligned(16))) float rsb_all[];   // [4][RS_TAPS - 1 + 960, padded to 4]
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x * 4 + w;
  if (b >= B) return;
  const int rate = __builtin_amdgcn_readfirstlane(rates[b]);
  const int di = rs_design_index(rate);
  const int id = ids[b];
  const int16_t* src = in + (size_t)b * in_stride;
  int16_t* dst = out + (size_t)b * out_stride;
  if (di < 0) {   // (wave-uniform)
    if (rate == 16000) {
      for (int i = lane; i < 320; i += 64) dst[i] = src[i];
    } else if (lane == 0) {
      atomicAdd(err, 1u);
    }
    if (ids_out && lane == 0) ids_out[b] = rate == 16000 ? id : -1;
    return;
  }
  if (ids_out && lane == 0) ids_out[b] = id;
  const int n_ext = rate / 50;
  const int n_in = dir == 0 ? n_ext : 320, n_out = dir == 0 ? 320 : n_ext;
  const bool vec = (in_stride & 7) == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0;   // (every n_in is a multiple of 8)
  rs_stream_pass(tab + dir * 3 + di, rsb_all + w * ((RS_H + 960 + 3) & ~3), lane, state, id, src, n_in, vec,
                 dst, n_out);
}

// Packed rows (lyra_hip_encode_streams_dev): resample_rates_kernel, dir 0, with row b at in + offsets[b] (offsets == nullptr:
// b * in_stride) inside a buffer of n_in_total samples.  A row whose offset is negative, no multiple of 8 samples (16 bytes)
// or whose [offset, offset + rates[b] / 50) leaves the buffer is treated as a row with an invalid rate: nothing of it is
// read, it writes nothing, is counted in *err and named -1 in ids_out.
__global__ __launch_bounds__(256) void resample_streams_kernel(const ResampleP* __restrict__ tab,
                                                                const int32_t* __restrict__ rates,
                                                                const int32_t* __restrict__ ids, int B,
                                                                uint8_t* __restrict__ state, const int16_t* __restrict__ in,
                                                                const int32_t* __restrict__ offsets, int in_stride,
                                                                long n_in_total, int16_t* __restrict__ out, int out_stride,
                                                                int32_t* __restrict__ ids_out, unsigned* __restrict__ err) {
  LYRA_STRESS(8);
  extern __shared__ __attribute__((aligned(16))) float rsb_all[];   // [4][RS_TAPS - 1 + 960, padded to 4]
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x * 4 + w;
  if (b >= B) return;
  const int rate = __builtin_amdgcn_readfirstlane(rates[b]);
  const int di = rs_design_index(rate);
  // (wave-uniform like the rate; said so, the slot's address costs no vector registers: 63, and 65 cost a wave -- DESIGN.md 4.4)
  const int id = __builtin_amdgcn_readfirstlane(ids[b]);
  const long off = offsets ? (long)__builtin_amdgcn_readfirstlane(offsets[b]) : (long)b * in_stride;
  const int n_in = rate / 50;
  const bool ok = (di >= 0 || rate == 16000) && off >= 0 && (off & 7) == 0 && off + n_in <= n_in_total;
  int16_t* dst = out + (size_t)b * out_stride;
  if (!ok) {   // (wave-uniform)
    if (lane == 0) {
      atomicAdd(err, 1u);
      if (ids_out) ids_out[b] = -1;
    }
    return;
  }
  const int16_t* src = in + off;
  if (ids_out && lane == 0) ids_out[b] = id;
  if (di < 0) {   // 16 kHz: no resampler (lyra_encoder.cc:59)
    for (int i = lane; i < 320; i += 64) dst[i] = src[i];
    return;
  }
  const bool vec = (reinterpret_cast<uintptr_t>(in) & 15) == 0;   // (every offset and every n_in is a multiple of 8)
  rs_stream_pass(tab + di, rsb_all + w * ((RS_H + 960 + 3) & ~3), lane, state, id, src, n_in, vec, dst, 320);
}

// The decode-direction twin (lyra_hip_decode_streams_dev): resample_rates_kernel, dir 1, with row b's rates[b] / 50 samples
// at out + offsets[b] (offsets == nullptr: b * out_stride) inside a buffer of n_out_total samples.  A row whose offset is
// negative, no multiple of 8 samples or whose [offset, offset + rates[b] / 50) leaves the buffer is treated as a row with
// an invalid rate: the test comes before anything of the row is read; the row writes nothing, its slot is neither read
// nor written, and it is counted in *err.
__global__ __launch_bounds__(256) void resample_streams_out_kernel(const ResampleP* __restrict__ tab,
                                                                    const int32_t* __restrict__ rates,
                                                                    const int32_t* __restrict__ ids, int B,
                                                                    uint8_t* __restrict__ state, const int16_t* __restrict__ in,
                                                                    int in_stride, int16_t* __restrict__ out,
                                                                    const int32_t* __restrict__ offsets, int out_stride,
                                                                    long n_out_total, unsigned* __restrict__ err) {
  LYRA_STRESS(8);
  extern __shared__ __attribute__((aligned(16))) float rsb_all[];   // [4][RS_TAPS - 1 + 960, padded to 4]
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x * 4 + w;
  if (b >= B) return;
  const int rate = __builtin_amdgcn_readfirstlane(rates[b]);
  const int di = rs_design_index(rate);
  const long off = offsets ? (long)__builtin_amdgcn_readfirstlane(offsets[b]) : (long)b * out_stride;
  const int n_out = rate / 50;
  const bool ok = (di >= 0 || rate == 16000) && off >= 0 && (off & 7) == 0 && off + n_out <= n_out_total;
  if (!ok) {   // (wave-uniform)
    if (lane == 0) atomicAdd(err, 1u);
    return;
  }
  const int16_t* src = in + (size_t)b * in_stride;
  int16_t* dst = out + off;
  if (di < 0) {   // 16 kHz: no resampler (lyra_decoder.cc:129), the hop itself
    for (int i = lane; i < 320; i += 64) dst[i] = src[i];
    return;
  }
  const bool vec = (in_stride & 7) == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0;   // (as resample_rates_kernel, dir 1)
  rs_stream_pass(tab + 3 + di, rsb_all + w * ((RS_H + 960 + 3) & ~3), lane, state, ids[b], src, 320, vec,
                 dst, n_out);
}

// =============================================================================================
// Device half of the batched LyraDecoder twin (host/lyra_batch_codec.cc).  The host runs the reference's per-stream
// state machine on integers only; the conditioned hops of the generative model and of the comfort-noise generator live
// in two [max_streams][320] arrays indexed by stream id, and each round's slices are assembled here.
// =============================================================================================
// dst[ids[b]][0..320) = src[b][0..320): a dense batch result into the by-id hop buffer (8 bytes per thread)
__global__ __launch_bounds__(128) void twin_scatter_kernel(const int16_t* __restrict__ src, const int32_t* __restrict__ ids,
                                                            int B, int16_t* __restrict__ dst) {
  LYRA_STRESS(10);
  const int b = blockIdx.x, t = threadIdx.x;
  if (t < 80) reinterpret_cast<uint2*>(dst + (size_t)ids[b] * 320)[t] = reinterpret_cast<const uint2*>(src + (size_t)b * 320)[t];
}
// One workgroup per slice.  RunModel slices + MaybeOverlapAndInsert (lyra_decoder.cc:342-373): where both hops
// contribute, sample i is (int16)(gan * w + cng * (1.f - w)) with w = fade_w[fade + i * fade_dir] -- the table holds
// (1.f + std::cos(fade * M_PI / 640)) / 2.f evaluated on the host in double exactly as the reference writes it, so the
// mix is bit-identical to the reference's on that host; float products and sum are separate roundings
// (-ffp-contract=off), the conversion truncates as the implicit float -> int16_t of push_back does.
// noise_row >= 0: this slice completes a RECEIVED hop -- its 320 samples are what noise_estimator_->ReceiveSamples has
// accumulated (:304-311); they are copied to row noise_row of the dense buffer the estimator kernel then reads.
__global__ __launch_bounds__(256) void twin_assemble_kernel(const TwinSlice* __restrict__ slices, int B,
                                                             const int16_t* __restrict__ gan,
                                                             const int16_t* __restrict__ cng,
                                                             const float* __restrict__ fade_w, int16_t* __restrict__ out,
                                                             int out_stride, int16_t* __restrict__ noise_dense) {
  LYRA_STRESS(10);
  const TwinSlice s = slices[blockIdx.x];
  const int n = s.gen_n > s.cng_n ? s.gen_n : s.cng_n;
  const int16_t* g = gan + (size_t)s.id * 320 + s.gan_off;
  const int16_t* c = cng + (size_t)s.id * 320 + s.cng_off;
  int16_t* o = out + (size_t)s.id * out_stride + s.out_off;
  for (int i = threadIdx.x; i < n; i += 256) {
    int16_t v;
    if (s.cng_n == 0) v = g[i];
    else if (s.gen_n == 0) v = c[i];
    else {
      const float w = fade_w[s.fade + i * s.fade_dir - TWIN_FADE_LO];
      const float a = (float)g[i] * w;
      const float b = (float)c[i] * (1.f - w);
      v = (int16_t)(int)(a + b);
    }
    o[i] = v;
  }
  if (s.noise_row >= 0)
    for (int i = threadIdx.x; i < 80; i += 256)
      reinterpret_cast<uint2*>(noise_dense + (size_t)s.noise_row * 320)[i] =
          reinterpret_cast<const uint2*>(gan + (size_t)s.id * 320)[i];
}

// =============================================================================================
// ComfortNoiseGenerator::AddFeatures + GenerateSamples(320) (lyra/comfort_noise_generator.cc:74-119): log-mel -> mel ->
// estimated FFT magnitudes -> random phase -> inverse STFT (FFT 1024, step 320) -> ClipToInt16.  Restated construction,
// counter-based phases, parity statement in oracle/lyra_oracle.c (lo_cng_generate) -- this kernel follows that function
// operation by operation in fp64 (same radix-2 butterflies and host-built twiddles as the log-mel kernel).
// features == nullptr: the stream's decoder-side noise estimate is used (lyra_decoder.cc:328-340).
// =============================================================================================
__global__ __launch_bounds__(256) void cng_kernel(const MelP* __restrict__ Pp, unsigned long long seed,
                                                   const int32_t* __restrict__ ids, int B,
                                                   uint8_t* __restrict__ state, const uint8_t* __restrict__ noise_state,
                                                   const float* __restrict__ features, int16_t* __restrict__ pcm) {
  LYRA_STRESS(9);
  const MelP& P = *Pp;
  extern __shared__ __attribute__((aligned(16))) double dsm[];
  double* re = dsm;
  double* im = dsm + 1024;
  double* mel = dsm + 2048;   // [160], then unused
  const int tid = threadIdx.x, b = blockIdx.x;
  const int id = ids[b];
  if (id < 0) return;   // masked row (lyra_hip_decode_lossy_dev: no comfort noise this tick): no output, no hop advance
  uint8_t* slot = state + (size_t)id * st::CNG_BYTES;
  const unsigned long long hop = *reinterpret_cast<const unsigned long long*>(slot + st::C_HOP);
  double* ola = reinterpret_cast<double*>(slot + st::C_OLA);
  const float* feat = features ? features + (size_t)b * 160
                               : reinterpret_cast<const float*>(noise_state + (size_t)id * st::NOISE_BYTES + st::N_EST);
  // (the slot key is zero unless the stream was imported from another id or context: state_layout.h C_KEY)
  const unsigned long long sd = seed ^ (unsigned long long)(unsigned)id ^ *reinterpret_cast<const unsigned long long*>(slot + st::C_KEY);
  cng_frame(P, tid, feat, sd, hop, re, im, mel);
  // window, overlap-add, emit the first 320 samples, shift the accumulator by one hop
  double acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = tid + 256 * q;
    acc[q] = ola[n] + cng_windowed(re, n);
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = tid + 256 * q;
    if (n < 320) {
      double y = acc[q];
      y = y < -32768.0 ? -32768.0 : (y > 32767.0 ? 32767.0 : y);   // ClipToInt16<double>
      pcm[(size_t)b * 320 + n] = (int16_t)y;
    } else {
      re[n - 320] = acc[q];   // staging for the shifted write-back
    }
  }
  __syncthreads();
  for (int n = tid; n < 1024; n += 256) ola[n] = n < 1024 - 320 ? re[n] : 0.0;
  if (tid == 0) *reinterpret_cast<unsigned long long*>(slot + st::C_HOP) = hop + 1;
}

// =============================================================================================
// state reset: zeros everywhere (the graphs' CALL_ONCE init subgraph assigns zero constants), int8
// histories hold the zero point of their tensor (== quantize(0.0f)); NoiseEstimator: is_noise_ = true
// (lyra/noise_estimator.cc:131).  One workgroup per stream walks that stream's slot in every region.
// =============================================================================================
__global__ __launch_bounds__(256) void reset_kernel(const ResetP* __restrict__ Pp, const int32_t* __restrict__ ids, int n, int all,
                                                     StateMap sm) {
  const ResetP& P = *Pp;
  const int sidx = blockIdx.x;
  if (sidx >= n) return;
  const int id = all ? sidx : ids[sidx];
#pragma unroll 1
  for (int r = 0; r < st::R_COUNT; ++r) {
    const int bytes = sm.bytes[r];   // (st::REGION_BYTES is a host-side table: no runtime indexing of it here)
    uint8_t* base = sm.base[r] + (size_t)id * bytes;
    for (int o = threadIdx.x * 16; o < bytes; o += 256 * 16) {
      const int v = reset_fill(P, r, o);
      const int w = (v & 255) * 0x01010101;
      i32x4 q = (i32x4){w, w, w, w};
      if ((r == st::R_NOISE_E || r == st::R_NOISE_D) && o == 0) q[st::N_IS_NOISE / 4] = 1;
      *reinterpret_cast<i32x4*>(base + o) = q;
    }
  }
}

}  // namespace lyra
