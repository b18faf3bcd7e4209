// kernels.h -- kernel parameter blocks and launch-side declarations (internal to liblyra_hip.so).
#pragma once
#include "lyra_dev.h"
#include "state_layout.h"

namespace lyra {

// ---- launch shapes and occupancy targets of the stage kernels ----------------------------------
constexpr int I8_WAVES = 4;       // waves per SIMD the int8 stage kernels are compiled for (5 -> at most 96 VGPRs)
constexpr int C64_WAVES = 4;      // waves per SIMD the 64-channel stage kernels are compiled for (3 -> up to 168 VGPRs, no spills)
constexpr int S0_STREAMS = 4;     // streams per workgroup of the 64-channel stages (4 with 256 threads, 8 with 512)
constexpr int S1_THREADS = 512;   // threads per tile of the 128-channel stages: 8 waves, 4 per SIMD with two tiles per CU
                                  // (256 = the 4-wave layout)

// ---- weight-ring depth (gemm_f32_core PFB) of the conv that closes each fp32 stage kernel -------
// These convs stream their weights from L2 at 0.25 B per MAC while the kernel's tiles finish one after the other; the
// depths come from the sweep in profiles/closing_convs_depth.txt (-D overrides: that sweep's builds).
#ifndef LYRA_PFB_ENC_S0
#define LYRA_PFB_ENC_S0 3
#endif
#ifndef LYRA_PFB_ENC_S1
#define LYRA_PFB_ENC_S1 3
#endif
#ifndef LYRA_PFB_DEC_S1
#define LYRA_PFB_DEC_S1 2
#endif
#ifndef LYRA_PFB_DEC_S2
#define LYRA_PFB_DEC_S2 4
#endif
constexpr int PFB_ENC_S0 = LYRA_PFB_ENC_S0, PFB_ENC_S1 = LYRA_PFB_ENC_S1, PFB_DEC_S1 = LYRA_PFB_DEC_S1,
              PFB_DEC_S2 = LYRA_PFB_DEC_S2;

// ---- encoder ---------------------------------------------------------------------------------
struct EncS0P { ConvF first; DwF dw[3]; ConvF pw[3]; ConvF cv[3]; ConvF down; WarmRange warm; };
struct EncS1P { DwF dw[3]; ConvF pw[3]; ConvF cv[3]; ConvF down; WarmRange warm; };
struct EncS2P {
  DwF dw0; ConvF pw0;
  QP q_r0, dq_r0, q_x1, out;
  LreluQ lr[7];
  const int8_t* lr_lut;    // [7][256]   lrelu_q tabulated (model.hip lrelu_luts)
  const int32_t* add_lut;  // [2][2][256] ADD operand rescalings
  ConvQ r0b;
  DwQ dwq[2]; ConvQ pwq[2]; ConvQ cvq[2]; AddQ add[2];
  ConvQ down2, bott;
  int mode;
  WarmRange warm;
};

// code_bytes: size of the kernel's own machine code to pull into L2 at start (lyra_dev.h code_warm; 0 = skip)
// tile0: first tile of this launch (workgroup i works on tile tile0 + i; api.hip tile_div)
__global__ void enc_s0_kernel(const EncS0P* P, const int16_t* pcm, const int32_t* ids, int B, uint8_t* state, float* out0,
                              int code_bytes, int tile0);
__global__ void enc_s1_kernel(const EncS1P* P, const float* in0, const int32_t* ids, int B, uint8_t* state, float* out1,
                              int code_bytes, int tile0);
__global__ void enc_s2_kernel(const EncS2P* P, const float* in1, const int32_t* ids, int B, uint8_t* state, float* feats,
                              float* codes_dbg, int code_bytes, int tile0);
__global__ void enc_s2_dr_kernel(const EncS2P* P, const float* in1, const int32_t* ids, int B, uint8_t* state,
                                 float* feats, float* codes_dbg, int code_bytes, int tile0);   // gemmlowp double rounding
__global__ void enc_s2_xn_kernel(const EncS2P* P, const float* in1, const int32_t* ids, int B, uint8_t* state,
                                 float* feats, float* codes_dbg, int code_bytes, int tile0);   // XNNPACK QS8 arithmetic (default)
__global__ void enc_s2_bm_kernel(const EncS2P* P, const float* in1, const int32_t* ids, int B, uint8_t* state,
                                 float* feats, float* codes_dbg, int code_bytes, int tile0);   // TFLite builtin kernels, per-operator mixture
__global__ void enc_side_kernel(const EncS0P* P0, const EncS1P* P1, const EncS2P* P2, const int16_t* pcm, const int32_t* ids,
                                int B, uint8_t* st0, uint8_t* st1, uint8_t* st2, float* e0, float* e1, float* feats,
                                float* codes_dbg, int code_bytes);
__global__ void enc_side_dr_kernel(const EncS0P* P0, const EncS1P* P1, const EncS2P* P2, const int16_t* pcm,
                                   const int32_t* ids, int B, uint8_t* st0, uint8_t* st1, uint8_t* st2, float* e0, float* e1,
                                   float* feats, float* codes_dbg, int code_bytes);
__global__ void enc_side_xn_kernel(const EncS0P* P0, const EncS1P* P1, const EncS2P* P2, const int16_t* pcm,
                                   const int32_t* ids, int B, uint8_t* st0, uint8_t* st1, uint8_t* st2, float* e0, float* e1,
                                   float* feats, float* codes_dbg, int code_bytes);
size_t enc_side_lds_bytes();
__global__ void enc_s12_xn_kernel(const EncS1P* P1, const EncS2P* P2, const float* e0, const int32_t* ids, int B, uint8_t* st1,
                                  uint8_t* st2, float* e1, float* feats, float* codes_dbg, int code_bytes);
size_t enc_s12_lds_bytes();
size_t enc_s0_lds_bytes(); int enc_s0_streams_per_wg(); int enc_s0_threads();
size_t enc_s1_lds_bytes(); int enc_s1_streams_per_wg(); int enc_s1_threads();
size_t enc_s2_lds_bytes(); int enc_s2_streams_per_wg();

// ---- decoder ---------------------------------------------------------------------------------
// int8 transpose conv k4/s2 as a GEMM [rows][K=128] x [K][N = 4 taps x 64]; N tiles ordered [co tile][tap].
// zfold[tap*64+co] = -zin * sum_c w[co][tap][c] (the GEMM runs on raw codes); bias added once per output row.
struct TconvQ { const i32x4* w; const int32_t* zfold; const int32_t* bias; int32_t M, sh, zout; };
struct DecS0P {
  ConvF head;                 // conv k3 g4 (fp32): 4 groups, K = 3 taps x 16, N = 128
  QP q0;                      // QUANTIZE after the float LeakyReLU
  TconvQ up0[4]; QP up0_dq[4]; const float* up0_sub[4];
  QP q1;                      // QUANTIZE of lrelu(x164)
  DwQ dwq[3]; ConvQ pwq[3]; ConvQ cvq[3];
  LreluQ lr[6]; AddQ add[2];
  const int8_t* lr_lut;       // [6][256]
  const int32_t* add_lut;     // [2][2][256]
  QP dq_r0, q3;               // DEQUANTIZE of resblock-0 conv out; QUANTIZE of (conv + float skip)
  TconvQ up1[2]; QP up1_dq[2]; const float* up1_sub[2];
  int mode;
  WarmRange warm;
};
struct DecS1P { DwF dw[3]; ConvF pw[3]; ConvF cv[3]; ConvF up; const float* up_sub; WarmRange warm; };
struct DecS2P { DwF dw[3]; ConvF pw[3]; ConvF cv[3]; ConvF up; float up_sub; WarmRange warm; };

__global__ void dec_s0_kernel(const DecS0P* P, const float* feats, const int32_t* ids, int B, uint8_t* state, float* out0,
                              const uint8_t* packets, int num_stages, const float* cb, int code_bytes, int tile0);
__global__ void dec_s0_dr_kernel(const DecS0P* P, const float* feats, const int32_t* ids, int B, uint8_t* state,
                                 float* out0, const uint8_t* packets, int num_stages, const float* cb, int code_bytes, int tile0);
__global__ void dec_s0_xn_kernel(const DecS0P* P, const float* feats, const int32_t* ids, int B, uint8_t* state,
                                 float* out0, const uint8_t* packets, int num_stages, const float* cb, int code_bytes, int tile0);
__global__ void dec_s0_bm_kernel(const DecS0P* P, const float* feats, const int32_t* ids, int B, uint8_t* state,
                                 float* out0, const uint8_t* packets, int num_stages, const float* cb, int code_bytes, int tile0);
__global__ void dec_s1_kernel(const DecS1P* P, const float* in0, const int32_t* ids, int B, uint8_t* state, float* out1,
                              int code_bytes, int tile0);
__global__ void dec_s2_kernel(const DecS2P* P, const float* in1, const int32_t* ids, int B, uint8_t* state, int16_t* pcm,
                              int code_bytes, int tile0);
__global__ void dec_side_kernel(const DecS0P* P0, const DecS1P* P1, const DecS2P* P2, const float* feats, const int32_t* ids,
                                int B, uint8_t* st0, uint8_t* st1, uint8_t* st2, float* d0, float* d1, int16_t* pcm,
                                const uint8_t* packets, int num_stages, const float* cb, int code_bytes);
__global__ void dec_side_dr_kernel(const DecS0P* P0, const DecS1P* P1, const DecS2P* P2, const float* feats,
                                   const int32_t* ids, int B, uint8_t* st0, uint8_t* st1, uint8_t* st2, float* d0, float* d1,
                                   int16_t* pcm, const uint8_t* packets, int num_stages, const float* cb, int code_bytes);
__global__ void dec_side_xn_kernel(const DecS0P* P0, const DecS1P* P1, const DecS2P* P2, const float* feats,
                                   const int32_t* ids, int B, uint8_t* st0, uint8_t* st1, uint8_t* st2, float* d0, float* d1,
                                   int16_t* pcm, const uint8_t* packets, int num_stages, const float* cb, int code_bytes);
size_t dec_side_lds_bytes();
__global__ void dec_s01_xn_kernel(const DecS0P* P0, const DecS1P* P1, const float* feats, const int32_t* ids, int B, uint8_t* st0,
                                  uint8_t* st1, float* d0, float* d1, const uint8_t* packets, int num_stages, const float* cb,
                                  int code_bytes);
size_t dec_s01_lds_bytes();
size_t dec_s0_lds_bytes(); int dec_s0_streams_per_wg();
size_t dec_s1_lds_bytes(); int dec_s1_streams_per_wg(); int dec_s1_threads();
size_t dec_s2_lds_bytes(); int dec_s2_streams_per_wg(); int dec_s2_threads();

// ---- RVQ / packets / log-mel / state ---------------------------------------------------------------
// cb: codebooks, natural layout [46][16][64]
// mask_ids (optional): frame i is skipped (empty packet, packet_bytes[i] = 0) where mask_ids[i] < 0
// cbn: [46][16] |c|^2 per codeword, then [46] 2^-14 max |c|^2 per stage (model.hip); stats (optional): [0] frame-stages that took
// the exact chain, [1] wavefront-stages that entered it
__global__ void rvq_encode_kernel(const float* cb, const float* cbn, const float* feats, int B, int num_stages, int32_t* indices,
                                  uint8_t* packets, const int32_t* mask_ids, int32_t* packet_bytes, unsigned* stats);
__global__ void rvq_encode_chain_kernel(const float* cb, const float* feats, int B, int num_stages, int32_t* indices,
                                  uint8_t* packets, const int32_t* mask_ids, int32_t* packet_bytes);
__global__ void rvq_encode_wide_kernel(const float* cb, const float* feats, int B, int num_stages, int32_t* indices,
                                  uint8_t* packets, const int32_t* mask_ids, int32_t* packet_bytes);
__global__ void rvq_decode_kernel(const float* cb, const int32_t* indices, const uint8_t* packets, int num_stages,
                                  int B, float* feats);
// mixed bitrates (lyra_hip_encode_mixed_dev / lyra_hip_decode_lossy_mixed_dev): packet rows MAX_PACKET_BYTES apart (lossy_plan.h).
// encode: frame i at bits[i] / 4 stages; an invalid bits[i] (not a multiple of 4 in 4..184) -> packet_bytes[i] = 0, row
// unwritten, counted in *err.  The tile runs to its largest stage count: stats counts those extra stages too.
__global__ void rvq_encode_mixed_kernel(const float* cb, const float* cbn, const float* feats, int B, const int32_t* bits,
                                        uint8_t* packets, const int32_t* mask_ids, int32_t* packet_bytes, unsigned* stats,
                                        unsigned* err);
// decode: row i at the stage count of its size pkt_bytes[i] (8 / 15 / 23 -> 16 / 30 / 46, else 0)
__global__ void rvq_decode_mixed_kernel(const float* cb, const uint8_t* packets, const int32_t* pkt_bytes, int bytes_from_bits,
                                        int B, float* feats);
struct MelP { const double* hann; const double* tw_re; const double* tw_im; const int* band; const double* w;
              const double* wsum;   // [160] total forward weight of every mel band (comfort-noise inverse mel)
              const double* tw4_re; const double* tw4_im;   // [768] W_1024^j, radix-4 log-mel FFT
              int start, end; };
// NoiseEstimator::Create's constants (noise_estimator.cc:96-124): round(1 s / 20 ms), 0.5^(20 ms / 0.7 s), 0.5^(20 ms / 1 s)
struct NoiseP { int hops_per_update; float max_smoothing, bound_decay; };
// std::exp(float) of the estimator (noise_update_wave, span_noise_scan_kernel): float(exp(double)), see misc_kernels.hip
__device__ __forceinline__ float expf_via_double(float x) {
  return (float)exp((double)x);
}
// noise_tail: continue with the NoiseEstimator update of the same hop (state must then be a NoiseEstimator region)
__global__ void logmel_kernel(const MelP* P, const int16_t* pcm, const int32_t* ids, int B, uint8_t* state, int stride,
                              int prev_off, float* mel, int noise_tail, NoiseP NP, int32_t* is_noise_out,
                              int32_t* masked_ids);
// the same with rows of id -1 skipped entirely (the estimator of lyra_hip_decode_lossy_dev sees received hops only)
__global__ void logmel_masked_kernel(const MelP* P, const int16_t* pcm, const int32_t* ids, int B, uint8_t* state, int stride,
                                     int prev_off, float* mel, int noise_tail, NoiseP NP, int32_t* is_noise_out,
                                     int32_t* masked_ids);
// per-stream sample rates (lyra_hip_encode_rates_dev): P4 = the four rates' MelP (8 / 16 / 32 / 48 kHz), np_tab the four NoiseP,
// rates[i] the rate of row i; rows of id -1 are skipped and named -1 in masked_ids
__global__ void logmel_rates_kernel(const MelP* P4, const int16_t* pcm, const int32_t* ids, const int32_t* rates, int B,
                                    uint8_t* state, int stride, int prev_off, const NoiseP* np_tab, int32_t* is_noise_out,
                                    int32_t* masked_ids);
size_t logmel_rates_lds_bytes();
// the same with DTX per row (lyra_hip_encode_streams_dev): a row with dtx[i] == 0 does not touch its estimator slot, keeps its
// id in masked_ids and is 0 in is_noise_out.  LDS logmel_rates_lds_bytes().
__global__ void logmel_streams_kernel(const MelP* P4, const int16_t* pcm, const int32_t* ids, const int32_t* rates,
                                      const int32_t* dtx, int B, uint8_t* state, int stride, int prev_off, const NoiseP* np_tab,
                                      int32_t* is_noise_out, int32_t* masked_ids);
__global__ void noise_update_kernel(NoiseP P, const int32_t* ids, int B, uint8_t* state, const float* mel,
                                    int32_t* is_noise_out, int32_t* masked_ids);
// Resampler (lyra/resampler.cc): out/in = up/down, coef[phase][tap] oldest tap first (oracle lo_resampler_design)
struct ResampleP { int up, down; float coef[3][40]; };
int resample_streams_per_wg();
size_t resample_lds_bytes(int n_in);
// in_stride / out_stride: samples between consecutive streams' rows (>= n_in / n_out: a chunk of longer rows)
__global__ void resample_kernel(ResampleP P, const int32_t* ids, int B, uint8_t* state, const int16_t* in, int n_in,
                                int in_stride, int16_t* out, int n_out, int out_stride);
// per-stream sample rates: tab [2][3] = [dir][8000, 32000, 48000]; dir 0: rates[b] -> 16 kHz, 1: 16 kHz -> rates[b]; a row at
// 16000 is copied (320 samples), any other non-codec rate writes nothing and is counted in *err; ids_out (optional):
// ids[b], or -1 for such a row
__global__ void resample_rates_kernel(const ResampleP* tab, int dir, const int32_t* rates, const int32_t* ids, int B,
                                      uint8_t* state, const int16_t* in, int in_stride, int16_t* out, int out_stride,
                                      int32_t* ids_out, unsigned* err);
size_t resample_rates_lds_bytes();
// resample_rates_kernel, dir 0, with packed rows: row b at in + offsets[b] samples (offsets null: b * in_stride) inside a
// buffer of n_in_total samples; a row with a bad offset or outside the buffer is treated as one with an invalid rate.
// LDS resample_rates_lds_bytes().
__global__ void resample_streams_kernel(const ResampleP* tab, const int32_t* rates, const int32_t* ids, int B, uint8_t* state,
                                        const int16_t* in, const int32_t* offsets, int in_stride, long n_in_total, int16_t* out,
                                        int out_stride, int32_t* ids_out, unsigned* err);
// resample_rates_kernel, dir 1, with packed rows (lyra_hip_decode_streams_dev): row b's rates[b] / 50 samples go to
// out + offsets[b] (offsets null: b * out_stride) inside a buffer of n_out_total samples; a row with a bad offset or outside
// the buffer is treated as one with an invalid rate (nothing written, slot untouched, counted in *err).
// LDS resample_rates_lds_bytes().
__global__ void resample_streams_out_kernel(const ResampleP* tab, const int32_t* rates, const int32_t* ids, int B, uint8_t* state,
                                            const int16_t* in, int in_stride, int16_t* out, const int32_t* offsets,
                                            int out_stride, long n_out_total, unsigned* err);
// ---- device half of BatchLyraDecoder (host/lyra_batch_codec.cc): hop buffers stay on the device, the host keeps ints --
// One slice of LyraDecoder::DecodeSamplesInternal's loop for one stream (lyra_decoder.cc:228-315): which samples of the
// conditioned generative-model hop and of the comfort-noise hop go where, and how they are cross-faded
// (MaybeOverlapAndInsert, :342-373).  Layout = lyra_hip_twin_slice (include/lyra_hip.h).
struct TwinSlice { int32_t id, gan_off, gen_n, cng_off, cng_n, fade, fade_dir, out_off, noise_row; };
constexpr int TWIN_FADE_LO = -640, TWIN_FADE_N = 1921;   // fade_progress range the weight table covers
__global__ void twin_scatter_kernel(const int16_t* src, const int32_t* ids, int B, int16_t* dst);
__global__ void twin_assemble_kernel(const TwinSlice* slices, int B, const int16_t* gan, const int16_t* cng,
                                     const float* fade_w, int16_t* out, int out_stride, int16_t* noise_dense);
// the counter-based phase generator of the comfort noise (cng_frame.h)
__device__ __forceinline__ unsigned long long splitmix64_dev(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__global__ void cng_kernel(const MelP* P, unsigned long long seed, const int32_t* ids, int B, uint8_t* state,
                           const uint8_t* noise_state, const float* features, int16_t* pcm);
__global__ void noise_read_kernel(const int32_t* ids, int B, const uint8_t* state, int field_off, float* out);
// ---- hop-synchronous packet loss (lossy_kernels.hip, lossy_plan.h; lyra_hip_decode_lossy_dev) -------------------------
// plan: the per-tick transition of every row; rx_ring_row / pkt_bytes may be null (all received / all packets whole)
__global__ void lossy_plan_kernel(const int32_t* ids, int B, const int32_t* pkt_bytes, int nbytes, const uint8_t* rx_ring_row,
                                  uint8_t* cng_state, int32_t* gen_ids, int32_t* cng_ids, int32_t* est_ids, int32_t* info,
                                  float* feats, unsigned* err);
// the same with the received rule of mixed bitrates (lossy_plan.h mixed_received)
__global__ void lossy_plan_mixed_kernel(const int32_t* ids, int B, const int32_t* pkt_bytes, int bytes_from_bits,
                                        const uint8_t* rx_ring_row, uint8_t* cng_state, int32_t* gen_ids, int32_t* cng_ids,
                                        int32_t* est_ids, int32_t* info, float* feats, unsigned* err);
// the tick's output hop per row (generative / comfort noise / cross-fade) + is_noise of unreceived rows + is_comfort_noise
__global__ void lossy_mix_kernel(const int32_t* ids, int B, const int32_t* info, const int16_t* gan, const int16_t* cng,
                                 const float* fade_w, int16_t* out, const uint8_t* noise_state, int32_t* is_noise,
                                 int32_t* is_cn);
// ---- conference bridge (bridge_kernels.hip; include/lyra_hip_bridge.h) --------------------------------------------------
// mix-minus over an inverted membership index: one wavefront per room, bad index entries skipped and counted in *err
__global__ void bridge_mix_kernel(const int16_t* pcm, int B, const int32_t* order, const int32_t* room_start, int n_rooms,
                                  int n_members, const int32_t* muted, const int32_t* is_cn, int16_t* mix, unsigned* err);
// ---- loudest-N speaker selection (speakers_kernels.hip; include/lyra_hip_speakers.h) --------------------------------------
// level[b] = sum of squares of row b (int64), for every row; zeroes row b of mix (where given), is_speaker[b], and pos_room[b]
// to -1; slot_of / row_room (shared encoders only, else nullptr): [b] to -1
__global__ void speakers_level_kernel(const int16_t* pcm, int B, long long* levels, int16_t* mix, int32_t* is_speaker,
                                      int32_t* pos_room, int n_members, int32_t* slot_of, int32_t* row_room);
// one wavefront per room over levels and the index only: the room's max_speakers loudest candidates into spk[room][8] (-1
// padded) and is_speaker, the room number of every position into pos_room; bad index entries counted in *err (here only)
__global__ void speakers_select_kernel(const long long* levels, int B, const int32_t* order, const int32_t* room_start,
                                       int n_rooms, int n_members, const int32_t* muted, const int32_t* is_cn,
                                       int max_speakers, unsigned long long* keys, int32_t* spk, int32_t* pos_room,
                                       int32_t* is_speaker, unsigned* err);
// one wavefront per 8 consecutive positions of the index: the sum of the room's speaker rows minus the listener's own
__global__ void speakers_mix_kernel(const int16_t* pcm, int B, const int32_t* order, int n_members, const int32_t* pos_room,
                                    int n_rooms, const int32_t* spk, int16_t* mix);
// ---- shared encoders (shared_bridge_kernels.hip; include/lyra_hip_shared_bridge.h) ----------------------------------------
// one wavefront per room behind speakers_select_kernel: the room's row of the slot table updated, the speaker row of every
// slot into slot_row[room][8], slot_of of the speakers, the room of every member row into row_room; a bad key counted in *err
__global__ void shared_slots_kernel(const int32_t* spk, const int32_t* stream_ids, int B, const int32_t* order,
                                    const int32_t* room_start, int n_rooms, int n_members, int max_speakers,
                                    const int32_t* room_keys, int n_table_rooms, int32_t* slots, int32_t* slot_row,
                                    int32_t* slot_of, int32_t* row_room, unsigned* err);
// one wavefront per encoder row e = room * (1 + N) + c: the sum of the room's speaker rows, minus the row in slot c - 1
__global__ void shared_mix_kernel(const int16_t* pcm, int B, int n_rooms, int max_speakers, const int32_t* spk,
                                  const int32_t* slot_row, const int32_t* room_keys, int n_table_rooms, int16_t* enc_mix);
// one thread per byte of the outgoing packets: row b receives the packet and size of its room's encoder row
__global__ void shared_fanout_kernel(int B, int n_rooms, int max_speakers, const int32_t* row_room, const int32_t* slot_of,
                                     const uint8_t* enc_packets, const int32_t* enc_packet_bytes, uint8_t* out_packets,
                                     int32_t* out_packet_bytes);
// ---- any request size up to one hop (decode_samples_kernels.hip, decode_samples_plan.h; lyra_hip_decode_samples_dev) ------
// plan: transition, id lists (-1: the row skips the leg), info [B][4], feature ring push / pop, features of starting hops
__global__ void ds_plan_kernel(const int32_t* ids, int B, const int32_t* pkt_bytes, int n_internal, uint8_t* cng_state,
                               int32_t* gen_ids, int32_t* cng1_ids, int32_t* cng2_ids, int32_t* est_ids, int32_t* info,
                               float* feats, float* ring, unsigned* err);
// the whole received hop of the rows whose hop completes -> est_in [B][320]
__global__ void ds_est_gather_kernel(const int32_t* ids, int B, const int32_t* info, const int16_t* gan_new,
                                     const int16_t* gan_held, int16_t* est_in);
// the row's passes (slices, cross-fade) -> out [B][out_stride]; new hops -> held hops; is_noise of rows without update; is_cn
__global__ void ds_slice_kernel(const int32_t* ids, int B, const int32_t* info, const int16_t* gan_new, const int16_t* cng_new,
                                int16_t* gan_held, int16_t* cng_held, const float* fade_w, int16_t* out, int out_stride,
                                const uint8_t* noise_state, int32_t* is_noise, int32_t* is_cn);
// lyra_hip_decode_samples_any_dev (decode_samples_any_kernels.hip): ds_plan_kernel for one round of a call of up to four hops,
// with the internal length per row: call [B][4] = {old leftover count, used, n_int, new count}, written in round 0
__global__ void ds_plan_any_kernel(const int32_t* ids, int B, const int32_t* pkt_bytes, int round, int n_ext, int rate,
                                   uint8_t* rs_state, int32_t* call, uint8_t* cng_state, int32_t* gen_ids, int32_t* cng1_ids,
                                   int32_t* cng2_ids, int32_t* est_ids, int32_t* info, float* feats, float* ring, unsigned* err);
// the end of such a call at 8 / 32 / 48 kHz: resampler over call[b][2] samples per row, old leftover + new samples -> out
// [B][n_ext], surplus -> the slot's leftover.  (The plan kernels' and the splice kernels' shared bodies: decode_samples_rows.h.)
size_t ds_splice_lds_bytes();
__global__ void ds_splice_kernel(ResampleP P, const int32_t* ids, int B, const int32_t* call, uint8_t* state, const int16_t* in,
                                 int in_stride, int16_t* out, int n_ext);
// lyra_hip_decode_samples_streams_dev (decode_samples_streams_kernels.hip): the two kernels above with the request size, the
// rate and the output offset per row.  call [B][DSS_CALL_WORDS] (decode_samples_streams_plan.h), written in round 0, which
// also validates the row and counts an invalid one in *rates_err; offsets null: row b at b * DSS_ROW_STRIDE
__global__ void ds_plan_streams_kernel(const int32_t* ids, int B, const int32_t* pkt_bytes, int round, const int32_t* rates,
                                       const int32_t* num_samples, const int32_t* offsets, int max_hops, long n_pcm_samples,
                                       uint8_t* rs_state, int32_t* call, uint8_t* cng_state, int32_t* gen_ids, int32_t* cng1_ids,
                                       int32_t* cng2_ids, int32_t* est_ids, int32_t* info, float* feats, float* ring,
                                       unsigned* err, unsigned* rates_err);
// tab: the context's [2][3] designs (rates_api.inc); a 16 kHz row is copied from `in`, an invalid row touches nothing; LDS of
// ds_splice_lds_bytes()
__global__ void ds_splice_streams_kernel(const ResampleP* tab, const int32_t* ids, int B, const int32_t* call, uint8_t* state,
                                         const int16_t* in, int in_stride, int16_t* out, const int32_t* offsets);
size_t logmel_lds_bytes();
size_t cng_lds_bytes();
struct ResetP { int8_t e_r2_1, e_r2_2, e_d2, e_bott, d_r0_0, d_r0_1, d_r0_2; };
// the byte that the 16 bytes at offset o of a slot of region r hold after a reset: zero, or the zero point of an int8 history
__device__ __forceinline__ int reset_fill(const ResetP& P, int r, int o) {
  if (r == st::R_E2) {
    if (o >= st::E_R2_1 && o < st::E_R2_2) return P.e_r2_1;
    if (o >= st::E_R2_2 && o < st::E_D2) return P.e_r2_2;
    if (o >= st::E_D2 && o < st::E_BOTT) return P.e_d2;
    if (o >= st::E_BOTT && o < st::E_BOTT + 2 * 512) return P.e_bott;
  } else if (r == st::R_D0) {
    if (o >= st::D_R0_0 && o < st::D_R0_1) return P.d_r0_0;
    if (o >= st::D_R0_1 && o < st::D_R0_2) return P.d_r0_1;
    if (o >= st::D_R0_2 && o < st::D_UP1) return P.d_r0_2;
  }
  return 0;
}
// region base pointers and per-stream slot sizes (state_layout.h), filled on the host, passed by value
struct StateMap { uint8_t* base[st::R_COUNT]; int bytes[st::R_COUNT]; };
__global__ void reset_kernel(const ResetP* P, const int32_t* ids, int n, int all, StateMap sm);
// ---- stream state as blobs (stream_state_kernels.hip, stream_blob.h; lyra_hip_export_streams / lyra_hip_import_streams) ----
// one workgroup per row of blobs [B][sb::BYTES]; ring / gan / cng: the by-id arrays of lyra_hip_decode_samples_dev (export:
// null = never allocated, the section is zero); import judges a row (sb::validate) before it writes, *err counts the refused
__global__ void state_export_kernel(const int32_t* ids, int B, int max_streams, StateMap sm, const float* ring,
                                    const int16_t* gan, const int16_t* cng, unsigned mode, unsigned long long seed,
                                    uint8_t* blobs);
__global__ void state_import_kernel(const int32_t* ids, int B, int max_streams, StateMap sm, float* ring, int16_t* gan,
                                    int16_t* cng, unsigned mode, unsigned long long seed, unsigned sides, const uint8_t* blobs,
                                    unsigned* err);
// ---- time-parallel spans (spans_kernels.hip, spans_plan.h; lyra_hip_encode_spans_dev / lyra_hip_decode_spans_dev) ----------
// One row of a span call's batch: stream `id` runs n_steps steps; step i reads buffer frame frame0 + i and, from step n_warm
// on, writes its output there.  Lanes (target >= 0) start from the reset state with target's ring phases + phase_add.
struct SpanRow { int32_t id, n_steps, n_warm, target, phase_add, handover; long long frame0; };
// step's rows between the frame-major buffer and the dense [B][row_bytes] rows of the stage kernels.  gather: frames -> dense,
// and step_ids[r] = the row's id while it runs, else -1; scatter: dense -> frames for the rows past their warm-up.
// unit16: rows are moved in 16-byte units (row_bytes a multiple of 16, both buffers 16-byte aligned), else byte by byte.
// map (optional; lyra_hip_encode_spans_dtx_dev): the rows count in a compacted frame list, index c is buffer frame map[c].
__global__ void span_gather_kernel(const SpanRow* rows, int B, int step, const uint8_t* frames, int row_bytes, int unit16,
                                   uint8_t* dense, int32_t* step_ids, const long long* map);
__global__ void span_scatter_kernel(const SpanRow* rows, int B, int step, const uint8_t* dense, int row_bytes, int unit16,
                                    uint8_t* frames, const long long* map);
// regions r0 .. r0 + 2 (R_E0 or R_D0) of rows[b].id: the reset state; ring phase words: target's + phase_add (target >= 0)
__global__ void span_lane_init_kernel(const ResetP* P, const SpanRow* rows, int n, int r0, StateMap sm);
// rows with handover != 0: regions r0 .. r0 + 2 of the lane -> the same regions of target
__global__ void span_handover_kernel(const SpanRow* rows, int n, int r0, StateMap sm);
// One span with frames of a call at 8 / 32 / 48 kHz: frames frame0 .. frame0 + n_frames - 1 of both PCM buffers belong to stream
// `id`; wg0 = the span's first workgroup of span_resample_kernel (four frames each; rows in rising wg0).  Uploaded behind the
// call's SpanRows, hence their size.
struct SpanRsRow { long long frame0, n_frames; int32_t id, wg0, pad[2]; };
static_assert(sizeof(SpanRsRow) == sizeof(SpanRow), "one upload holds both kinds of row");
// The row of workgroup wg where the grid is the workgroups of all rows (SpanRsRow, SpanDtxRow, SpanLossyRow): the last row whose
// first workgroup (member wg0) is not behind wg; rows in rising wg0, rows[0].*wg0 == 0, n_rows >= 1.  Scalar work: blockIdx alone.
template <typename Row>
__device__ __forceinline__ int span_row_of_workgroup(const Row* rows, int n_rows, int32_t Row::*wg0, int wg) {
  int lo = 0, hi = n_rows - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[mid].*wg0 <= wg) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// in [frames][n_in] -> out [frames][n_out] for the frames of the rows' spans, with the design P (n_out = n_in * up / down);
// state = the resampler region of the side (R_RS_E / R_RS_D): read and written by each span's frame 0 only (the phase word is
// read by all).  grid = the workgroups of all rows, 256 threads, LDS resample_lds_bytes(n_in).
__global__ void span_resample_kernel(ResampleP P, const SpanRsRow* rows, int n_rows, uint8_t* state, const int16_t* in, int n_in,
                                     int16_t* out, int n_out);
// ---- DTX on spans (spans_dtx_kernels.hip; lyra_hip_encode_spans_dtx_dev / lyra_hip_noise_spans_dev) --------------------------
// One span with frames: buffer frames frame0 .. frame0 + n_frames - 1 belong to stream `id`; wg0 = the span's first workgroup of
// span_logmel_kernel (two frames each; rows in rising wg0); region = the frames of the rows in front of it: where the span's mel
// rows and its part of the map start.
struct SpanDtxRow { long long frame0, n_frames; int32_t id, wg0; long long region; };
static_assert(sizeof(SpanDtxRow) == sizeof(SpanRow), "one upload holds both kinds of row");
constexpr int SPAN_MEL_ROW = 164;   // floats per mel row: 160 bins, Average() of them, padding to 16 bytes
// log-mel of every frame of every row's span -> mel[region + f][SPAN_MEL_ROW]; state = a NoiseEstimator region, of which only
// N_PREV is read (frame 0) and written (the span's last frame), both by the span's first workgroup.  grid = the workgroups
// of all rows, 256 threads, LDS logmel_lds_bytes().
__global__ void span_logmel_kernel(const MelP* P, const SpanDtxRow* rows, int n_rows, uint8_t* state, const int16_t* pcm,
                                   float* mel);
// NoiseEstimator::ReceiveSamples' decision + recurrence over the frames of one span per wavefront (grid n_rows, 64 threads):
// flag_out[frame] = v_noise / v_active, map[region + c] = buffer frame of the span's c-th non-noise frame (map optional),
// counts[row] = the span's non-noise frames.
__global__ void span_noise_scan_kernel(NoiseP P, const SpanDtxRow* rows, int n_rows, uint8_t* state, const float* mel,
                                       int32_t* flag_out, int v_noise, int v_active, long long* map, int32_t* counts);

// ---- packet loss on spans (spans_lossy_kernels.hip, spans_lossy_plan.h; lyra_hip_decode_spans_lossy_dev) -------------------
// One span with frames.  Its parts of the call's dense lists: received ticks rx0 .. rx0 + n_rx - 1 (SpanLossyRx, and the mel rows),
// run_cng ticks cng0 .. (SpanLossyCng), frames info0 .. (SpanLossyFrame); rx_wg0 / cng_wg0: the span's first workgroup of
// span_logmel_map_kernel (two received frames each) / span_cng_kernel (one tick each), rows in rising order of both;
// snap_v0: the snapshot row of the estimate on entry, or -1; ctl_out: the control word after the span.
struct SpanLossyRow {
  long long frame0, n_frames, info0;
  int32_t id, rx0, n_rx, rx_wg0, cng0, n_cng, cng_wg0, snap_v0;
  uint32_t ctl_out;
  int32_t pad;
};
static_assert(sizeof(SpanLossyRow) == 2 * sizeof(SpanRow), "two row slots of the upload");
struct SpanLossyRx { long long frame; int32_t snap, pad; };     // a received tick: its buffer frame; the snapshot row that takes the estimate after it, or -1
struct SpanLossyCng { long long frame; int32_t snap, info; };   // a run_cng tick: its buffer frame, the snapshot row it reads, lossy_info
struct SpanLossyFrame { int32_t info, back; };                  // a frame: lossy_info; frames back to the last received one (0: none in the span)
__global__ void span_lossy_ctl_read_kernel(int32_t* io, int n, int max_streams, const uint8_t* cng_state);
__global__ void span_lossy_feat_kernel(const SpanRow* rows, int B, int step, const uint8_t* gen_received, float* feats);
// grid = the workgroups of all rows, 256 threads, LDS logmel_lds_bytes(); state: the decoder-side NoiseEstimator region
__global__ void span_logmel_map_kernel(const MelP* P, const SpanLossyRow* rows, int n_rows, uint8_t* state, const SpanLossyRx* rx,
                                       const int16_t* pcm, float* mel);
// grid n_rows, 64 threads
__global__ void span_lossy_scan_kernel(NoiseP P, const SpanLossyRow* rows, int n_rows, uint8_t* state, const float* mel,
                                       const SpanLossyRx* rx, int32_t* is_noise_out, float* snaps, int32_t* entry_noise);
// final == 0: grid = the run_cng ticks of all rows; final != 0: grid n_rows, behind the first launch.  256 threads, LDS cng_lds_bytes()
__global__ void span_cng_kernel(const MelP* P, unsigned long long seed, const SpanLossyRow* rows, int n_rows, int final,
                                uint8_t* state, const SpanLossyCng* ticks, const float* snaps, const float* fade_w, int16_t* pcm16);
// grid = ceil(total / 256): one thread per frame of the rows
__global__ void span_lossy_finish_kernel(const SpanLossyRow* rows, int n_rows, long long total, const SpanLossyFrame* frames,
                                         uint8_t* cng_state, const int32_t* entry_noise, int32_t* is_noise, int32_t* is_cn);

// ---- per-frame bitrates on spans (spans_mixed_kernels.hip; lyra_hip_encode_spans_mixed_dev / lyra_hip_decode_spans_lossy_mixed_dev)
// span_gather_kernel's movement plus one int32 per dense row, step_size[r], for the mixed quantizer kernels.  grid as the
// uniform gather's: 40 units per row (encode) or MAX_PACKET_BYTES (decode), 256 threads.
//   frame_bits != null (encode): frames = PCM [frames][640] in 16-byte units; step_size[r] = frame_bits[buffer frame], and 4 for
//     a row that has ended (rvq_encode_mixed_kernel counts an invalid bit count of every row < B, masked or not);
//   else (decode): frames = packets [frames][MAX_PACKET_BYTES]; step_size[r] = tick_bytes[row.frame0 + step] (the compacted
//     index itself), that many bytes of the row move, and 0 for a row that has ended.
__global__ void span_gather_mixed_kernel(const SpanRow* rows, int B, int step, const uint8_t* frames, const int32_t* frame_bits,
                                         const uint8_t* tick_bytes, uint8_t* dense, int32_t* step_ids, int32_t* step_size,
                                         const long long* map);
// dense [B][MAX_PACKET_BYTES] -> frames [frames][MAX_PACKET_BYTES] for the rows past their warm-up: the first
// (step_bits[r] + 7) / 8 bytes of the row, and packet_bytes[frame] = that size.  grid: MAX_PACKET_BYTES units per row.
__global__ void span_scatter_mixed_kernel(const SpanRow* rows, int B, int step, const uint8_t* dense, const int32_t* step_bits,
                                          uint8_t* frames, int32_t* packet_bytes, const long long* map);

// ---- per-span sample rates on spans (spans_rates_kernels.hip; include/lyra_hip_spans_rates.h) ---------------------------------
// The passes over every frame of a call with the rate looked up per row: SpanRsRow::pad[0] holds the span's rate (8000 / 16000 /
// 32000 / 48000), and the estimator's kernels read it from rate_rows[i] for their row i (one row per span with frames in both).
// span_resample_kernel with tab = the [2][3] designs of resample_rates_kernel; dir 0: in = external rate, rows in_stride apart
// with rate / 50 samples each, out = 16 kHz; dir 1 the reverse.  A 16 kHz row is copied and touches no slot.  grid and block as
// span_resample_kernel, LDS resample_rates_lds_bytes().
__global__ void span_resample_rates_kernel(const ResampleP* tab, int dir, const SpanRsRow* rows, int n_rows, uint8_t* state,
                                           const int16_t* in, int in_stride, int16_t* out, int out_stride);
// span_logmel_kernel / span_noise_scan_kernel with P4 = the four rates' MelP, np_tab = the four rates' NoiseP
__global__ void span_logmel_rates_kernel(const MelP* P4, const SpanDtxRow* rows, const SpanRsRow* rate_rows, int n_rows,
                                         uint8_t* state, const int16_t* pcm, float* mel);
__global__ void span_noise_scan_rates_kernel(const NoiseP* np_tab, const SpanDtxRow* rows, const SpanRsRow* rate_rows, int n_rows,
                                             uint8_t* state, const float* mel, int32_t* flag_out, int v_noise, int v_active,
                                             long long* map, int32_t* counts);

// ---- per-span sample rates on a packed external-rate buffer (spans_packed_kernels.hip; include/lyra_hip_spans_packed.h) --------
// span_resample_rates_kernel with the external-rate side one flat array: SpanRsRow::pad[1] holds the span's base in units of 8
// samples, frame f of the span lies at pad[1] * 8 + f * (rate / 50); the 16 kHz side stays [frames][320] by buffer frame.
// dir 0: in = external rate, out = 16 kHz; dir 1 the reverse.  grid, block and LDS as span_resample_rates_kernel.
__global__ void span_resample_packed_kernel(const ResampleP* tab, int dir, const SpanRsRow* rows, int n_rows, uint8_t* state,
                                            const int16_t* in, int16_t* out);

}  // namespace lyra
