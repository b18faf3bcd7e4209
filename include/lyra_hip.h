/*
 * lyra_hip.h -- C ABI of the MI355X-native Lyra encode/decode hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * Each entry point names the reference interface it replaces (file:line
 * relative to the google/lyra v1.3.2 tree).  The C++ plugin adapters in
 * lyra_amd/host/ (FeatureExtractorInterface / VectorQuantizerInterface /
 * GenerativeModelInterface) and the Python mirror lyra_amd/codec.py are thin
 * callers of these functions; INTEGRATION.md shows the binding a reference
 * maintainer would add in lyra/lyra_components.cc:42-65.
 *
 * Model: one context = one GPU + four HIP streams (encode side / decode side / quantizer / decoder-side
 * noise estimator, see "Streams") + per-stream codec state for `max_streams` independent audio
 * streams.  A "frame" is one 20 ms hop of
 * 16 kHz audio (320 samples); the codec is streaming/causal, so stream `id`
 * must be fed its frames in order (the reference keeps this state inside the
 * TFLite interpreter's resource variables: lyra/tflite_model_wrapper.cc:36-121).
 *
 * Threading: calls on one context must be serialised by the caller (as for one
 * reference codec object); distinct contexts are independent.  A batch must not
 * name the same stream id twice (two frames of one stream in a call would race on its state): host-pointer variants
 * reject it with LYRA_HIP_EINVAL, `_dev` variants cannot look at the ids and rely on the caller.
 * All functions return 0 on success or a
 * negative LYRA_HIP_E* code; lyra_hip_last_error() describes the last failure.
 * There is NO CPU fallback: creating a context without a usable gfx950 device
 * fails.
 *
 * Pointer flavours: functions without suffix take HOST pointers (they copy
 * H2D/D2H and synchronise); `_dev` variants take DEVICE pointers, enqueue and
 * do not synchronise.
 *
 * Streams: a context runs four HIP streams -- the ENCODE side (extract,
 * rvq_encode, the feature extractor of encode), the DECODE side (rvq_decode,
 * generate, decode, logmel; the stateless helpers rvq_decode_dev / logmel_dev
 * count as decode-side calls too) and one for the quantizer of
 * lyra_hip_encode_dev / lyra_hip_encode_dtx_dev, which starts once the call's
 * features are ready and runs underneath the next call's feature extractor and
 * the previous call's decoder (a 46-stage dependent chain that would leave the
 * chip nearly idle if anything queued behind it), and one for the decoder-side
 * NoiseEstimator of lyra_hip_noise_receive_dev, which runs behind the decoder's
 * last stage underneath the next step.  Encoder and decoder state are disjoint.
 * What the library guarantees on the GPU, without any caller synchronisation:
 *   (1) a decode-side call is ordered after EVERY earlier encode-side call, so
 *       encode_dev -> decode_dev on the produced packets just works;
 *   (2) the outputs of an encode-side call are written after every earlier
 *       decode-side call EXCEPT (at most) THE MOST RECENT ONE has finished:
 *       encode of frame i+1 overlaps decode of frame i, but its packets never
 *       overtake the decode of frame i-1;
 *   (3) calls of one side apply to a stream's state in call order, whatever the
 *       order in which a call lists its streams -- also on a context that splits
 *       batches over several stream sets (LYRA_HIP_SUBBATCHES > 1: every split
 *       call then waits for all chunks of the previous call of its side; only
 *       inside lyra_hip_run_steps_dev, which has one id list for all its steps,
 *       do the chunks run as independent pipelines).
 * Two-buffer rule for `_dev` callers: alternate two packet/PCM buffer sets
 * (step i uses set i & 1).  By (2) the encode that rewrites set i & 1 at step
 * i+2 is ordered after the decode that read it at step i.  A caller that
 * reuses ONE buffer set must lyra_hip_synchronize() (or lyra_hip_set_serial)
 * between steps.
 * Small contexts (max_streams <= 1024) partition the chip: the encode-side and
 * quantizer streams run on one half of every XCD's CUs, the decode-side and
 * noise-estimator streams on the other (CU-masked streams).  At such batches a
 * stage kernel is 64-256 workgroups on 256 CUs and two concurrent dispatches
 * are placed independently of each other -- some CUs get two tiles, some none,
 * and a kernel lasts as long as its slowest tile; kept apart, config #2
 * (1,024 streams) gains 10 %.  Larger contexts share the whole chip (each chain
 * wants all of it in turn); LYRA_HIP_CU_MASKS overrides either way.
 * The library streams are hipStreamNonBlocking (CU-masked ones, created through
 * hipExtStreamCreateWithCUMask, are ordinary blocking streams with respect to
 * the NULL stream): they do NOT order against the
 * null stream or any stream of the caller.  A `_dev` caller that produces
 * inputs or consumes outputs on its own stream brackets the calls with
 * lyra_hip_wait_for_stream(ctx, s) (library work enqueued afterwards waits
 * for what is already enqueued on s) and lyra_hip_stream_wait(ctx, s) (work
 * enqueued on s afterwards waits for the library work enqueued so far), or
 * synchronises.  `_dev` calls run on the context's device regardless of the
 * caller's current device (which is restored on return).
 */
#ifndef LYRA_HIP_H_
#define LYRA_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LYRA_HIP_HOP 320          /* samples per 20 ms frame at 16 kHz (lyra_config.h:70-168) */
#define LYRA_HIP_NUM_FEATURES 64  /* kNumFeatures */
#define LYRA_HIP_NUM_MEL 160      /* kNumMelBins */
#define LYRA_HIP_MAX_STAGES 46    /* 184 bits / 4 bits per RVQ stage (lyra_config.cc:44-48) */

#define LYRA_HIP_EINVAL (-1)   /* bad argument (bit count, batch size, stream id, null pointer) */
#define LYRA_HIP_ENODEV (-2)   /* no usable gfx950 device */
#define LYRA_HIP_EMODEL (-3)   /* model directory / weight container unreadable or wrong version */
#define LYRA_HIP_EHIP (-4)     /* HIP runtime error */
#define LYRA_HIP_ENOMEM (-5)

/* Arithmetic flavour of the graphs' int8 regions (oracle/lyra_oracle.c header):
 *   XNNPACK          what the reference runs -- it executes both graphs through TFLite's XNNPACK delegate
 *                    (soundstream_encoder.cc:39-40, lyra_gan_model.cc:39-40, tflite_model_wrapper.cc:63-85): QS8 convolutions
 *                    requantised in fp32, XNNPACK's own int8 LeakyReLU / ADD / QUANTIZE kernels.  Every formula is held
 *                    against real XNNPACK code (tests/test_xnnpack_witness.py).  The default.
 *   EXACT, GEMMLOWP_DOUBLE
 *                    TFLite's builtin kernels (what the reference falls back to when the delegate cannot be applied,
 *                    tflite_model_wrapper.cc:76-78): Q31 single-rounding or gemmlowp double-rounding convolutions, gemmlowp
 *                    LeakyReLU / ADD, round-half-away QUANTIZE.
 *   BUILTIN_MIXED    what the graphs compute if the delegate takes the fp32 operators but NOT the signed-int8 ones: the
 *                    reference ORs in only TFLITE_XNNPACK_DELEGATE_FLAG_QU8 (tflite_model_wrapper.cc:65-67) and its graphs are
 *                    QS8, so whether the int8 regions reach XNNPACK depends on a build-time default of TFLite 2.11's delegate
 *                    that cannot be observed offline.  TFLite's builtin int8 kernels per operator: ungrouped
 *                    CONV_2D single rounding, grouped CONV_2D / DEPTHWISE_CONV_2D / TRANSPOSE_CONV double rounding, builtin
 *                    LeakyReLU / ADD / QUANTIZE.  Whichever way that default falls, a bit-exact mode exists; switching is this
 *                    one argument.
 * The fp32 layers are the same in all four: bias-first fused chains (XNNPACK's order). */
#define LYRA_HIP_REQUANT_EXACT 0
#define LYRA_HIP_REQUANT_GEMMLOWP_DOUBLE 1
#define LYRA_HIP_REQUANT_XNNPACK 2
#define LYRA_HIP_REQUANT_BUILTIN_MIXED 3
#define LYRA_HIP_REQUANT_DEFAULT LYRA_HIP_REQUANT_XNNPACK

typedef struct lyra_hip_ctx lyra_hip_ctx;

/* Replaces CreateFeatureExtractor / CreateQuantizer / CreateGenerativeModel
 * (lyra/lyra_components.cc:42-55) + TfLiteModelWrapper::Create
 * (lyra/tflite_model_wrapper.cc:36-95).  `model_dir` is either the reference's
 * own model directory (soundstream_encoder.tflite, quantizer.tflite,
 * lyragan.tflite, lyra_config.binarypb -- converted in memory) or a directory
 * holding the pre-packed lyra_v1.lyrapack (tools/pack_weights.py / pack_tool
 * output for that directory; used first if present).  Version identifier 3 as
 * lyra_config.h:145-166.  The container is validated (bounds, dtypes, the
 * layer shapes the kernels are specialised to): a truncated or foreign file
 * gives LYRA_HIP_EMODEL.
 * Developer switches read from the environment here (results are bit-identical
 * either way):
 *   LYRA_HIP_SUBBATCHES=<n>  split every `_dev` call into n sub-batches on stream
 *                            sets of their own (pays when only one side is driven:
 *                            decode-only at B = 8192 +6 % with n = 2; default 1).
 *                            Calls that are not split (resample, noise estimator,
 *                            small batches ...) are ordered after every chunk of
 *                            the split call before them and vice versa;
 *   LYRA_HIP_FUSED=<mask>    (variant build `make parked` only) bit 0: the encoder side as one
 *                            launch instead of three, bit 1: the decoder side likewise, bit 2: encoder
 *                            stages 1 + 2 as one launch, bit 3: decoder stages 0 + 1 (all slower at
 *                            B = 4096; default 0);
 *   LYRA_HIP_RVQ_WIDE=1      the 104 KB / 244-VGPR quantizer kernel;
 *   LYRA_HIP_CU_MASKS=e,d,q,n  CU-mask patterns (32-bit hex, repeated over the chip) of the encode / decode / quantizer /
 *                            noise streams; 0 = no mask (default: 00ff00ff,ff00ff00,00ff00ff,ff00ff00 when
 *                            max_streams <= 1024, none above);
 *   LYRA_HIP_PRIO=e,d,q      stream priorities of the encode / decode / quantizer streams (0 lowest .. 2 highest;
 *                            default 0,0,2: the two chains equal, the small quantizer first; 0,2,0 = rounds 2-3:
 *                            decoder chain first -- better for blocking decode calls beside an encoder, bimodal for the `_dev` pipeline);
 *   LYRA_HIP_TILE_DIV_<K>=k  launch stage kernel K (ENC_S0 .. DEC_S2) as k slices of its tiles. */
/* max_streams: 1 .. 289,262 per context (per-stream state is addressed with 32-bit byte offsets; 83 KB of state per stream,
 * so that is 24 GB of the 288 -- more streams: more contexts). */
int lyra_hip_create(const char* model_dir, int device, int max_streams, int requant_mode, lyra_hip_ctx** out);
/* The same from an in-memory lyra_v1.lyrapack image (e.g. read once by rank 0 and broadcast to the other GPUs' ranks
 * over RCCL); the image is copied, the caller keeps ownership. */
int lyra_hip_create_from_image(const void* image, size_t image_bytes, int device, int max_streams, int requant_mode,
                               lyra_hip_ctx** out);
void lyra_hip_destroy(lyra_hip_ctx* ctx);
const char* lyra_hip_last_error(const lyra_hip_ctx* ctx); /* ctx may be NULL: last create() error */

/* Replaces TfLiteModelWrapper::ResetVariableTensors (tflite_model_wrapper.cc:111-113) /
 * constructing fresh codec objects.  ids == NULL resets every stream. */
int lyra_hip_reset_streams(lyra_hip_ctx* ctx, const int32_t* stream_ids, int n);

/* ---- per-plugin entry points (the three reference interfaces) -------------------------------- */

/* FeatureExtractorInterface::Extract as implemented by SoundStreamEncoder::Extract
 * (lyra/soundstream_encoder.cc:53-64): pcm [B][320] int16 -> features [B][64] f32. */
int lyra_hip_extract(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B, const int16_t* pcm, float* features);

/* VectorQuantizerInterface::Quantize (lyra/residual_vector_quantizer.cc:77-110), stateless:
 * features [B][64] -> indices [B][46] int32 (-1 beyond num_bits/4 stages).  num_bits <= 184, % 4 == 0. */
int lyra_hip_rvq_encode(lyra_hip_ctx* ctx, int B, const float* features, int num_bits, int32_t* indices);

/* VectorQuantizerInterface::DecodeToLossyFeatures (residual_vector_quantizer.cc:112-168), stateless:
 * indices [B][46] (-1 = unused stage) -> lossy features [B][64]. */
int lyra_hip_rvq_decode(lyra_hip_ctx* ctx, int B, const int32_t* indices, float* features);

/* GenerativeModel::AddFeatures + GenerateSamples(320) as implemented by LyraGanModel
 * (lyra/generative_model_interface.h:50-101, lyra/lyra_gan_model.cc:53-64):
 * features [B][64] -> pcm [B][320] int16 (x32768, clamp, truncate: dsp_utils.h:54-88). */
int lyra_hip_generate(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B, const float* features, int16_t* pcm);

/* FeatureExtractorInterface::Extract as implemented by LogMelSpectrogramExtractorImpl::Extract
 * (lyra/log_mel_spectrogram_extractor_impl.cc:96-126), the NoiseEstimator front end
 * (noise_estimator.cc:157-160): pcm [B][320] int16 -> log-mel [B][160] f32.  Keeps its own
 * per-stream 320-sample history. */
int lyra_hip_logmel(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B, const int16_t* pcm, float* mel);

/* NoiseEstimator (lyra/noise_estimator.h:45-60), one instance per stream and side: side LYRA_HIP_SIDE_ENCODER is the
 * estimator LyraEncoder owns for DTX (lyra_encoder.cc:81-83), LYRA_HIP_SIDE_DECODER the one LyraDecoder feeds with every
 * decoded hop of a received packet (lyra_decoder.cc:304-311).  noise_receive = ReceiveSamples for one full 320-sample
 * hop per stream (its own log-mel front end + ComputeIsNoise + DecayBounds / UpdateNoiseEstimate,
 * noise_estimator.cc:144-245) and returns is_noise() per stream (int32 0/1); noise_estimate = noise_estimate(),
 * [B][160] log-mel bins. */
#define LYRA_HIP_SIDE_ENCODER 0
#define LYRA_HIP_SIDE_DECODER 1
int lyra_hip_noise_receive(lyra_hip_ctx* ctx, int side, const int32_t* stream_ids, int B, const int16_t* pcm,
                           int32_t* is_noise);
int lyra_hip_noise_estimate(lyra_hip_ctx* ctx, int side, const int32_t* stream_ids, int B, float* estimate);

/* Resampler::Resample (lyra/resampler.cc:57-62), one instance per stream and side: LYRA_HIP_SIDE_ENCODER is the
 * resampler LyraEncoder applies to incoming audio (external rate -> 16 kHz, lyra_encoder.cc:59-66,119-122),
 * LYRA_HIP_SIDE_DECODER the one behind LyraDecoder's BufferedResampler (16 kHz -> external, lyra_decoder.cc:107-113).
 * in [B][n_in] int16 -> out [B][n_in * out_rate / in_rate]; rates from {8000, 16000, 32000, 48000}, one of them
 * 16000; n_in <= 960 and a multiple of in_rate / gcd.  audio_dsp::QResampler is restated (Kaiser-windowed sinc,
 * radius 17 input samples, primed: output delayed by 17 input samples); see oracle/lyra_oracle.c for the parity note. */
int lyra_hip_resample(lyra_hip_ctx* ctx, int side, const int32_t* stream_ids, int B, const int16_t* in, int n_in,
                      int in_rate, int out_rate, int16_t* out);

/* ComfortNoiseGenerator::AddFeatures + GenerateSamples(320) (lyra/comfort_noise_generator.cc:74-119): one 20 ms hop
 * of noise per stream whose 160-bin log-mel matches `features` [B][160]; features == NULL uses each stream's decoder-side
 * noise estimate, as LyraDecoder::RunComfortNoiseGenerator does (lyra_decoder.cc:328-340).  Phases come from a
 * counter-based generator (seed, stream id, hop, bin) instead of the reference's non-deterministic absl::BitGen. */
int lyra_hip_comfort_noise(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B, const float* features, int16_t* pcm);
int lyra_hip_set_cng_seed(lyra_hip_ctx* ctx, uint64_t seed);
/* The sample rate LyraEncoder::Create was called with, for the ENCODER-side noise estimator of the calls that follow
 * (lyra_hip_encode_dtx[_dev], lyra_hip_noise_receive[_dev] side ENCODER): the reference hands NoiseEstimator::Create
 * its external rate together with the internal 320-sample hop (lyra_encoder.cc:82-85), so the estimator's update period
 * and half-lives, counted in hops, depend on it (noise_estimator.cc:96-124).  8000 / 16000 (default) / 32000 / 48000.
 * A host-side setting read at enqueue time: set it before each call when encoders of different rates share a context. */
int lyra_hip_set_encoder_sample_rate(lyra_hip_ctx* ctx, int sample_rate_hz);

/* ---- fused paths -------------------------------------------------------------------------------- */

/* LyraEncoder::Encode without resampling/DTX (lyra/lyra_encoder.cc:143-155): Extract -> Quantize ->
 * Packet<>::PackQuantized (lyra/packet.h:91-122, zero header bits).
 * pcm [B][320] -> packets [B][num_bits/8 rounded up] (8 / 15 / 23 bytes for 64 / 120 / 184 bits). */
int lyra_hip_encode(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B, const int16_t* pcm, int num_bits,
                    uint8_t* packets);

/* LyraEncoder::Encode with enable_dtx = true (lyra/lyra_encoder.cc:131-156): every hop updates the stream's
 * encoder-side NoiseEstimator; a hop that is noise yields an EMPTY packet (packet_bytes[i] = 0, the packet row is left
 * zero) and does not run the feature extractor, so the encoder state of that stream does not advance; any other hop
 * is encoded as lyra_hip_encode does (packet_bytes[i] = num_bits / 8 rounded up). */
int lyra_hip_encode_dtx(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B, const int16_t* pcm, int num_bits,
                        uint8_t* packets, int32_t* packet_bytes);

/* LyraDecoder::SetEncodedPacket + DecodeSamples(320) steady state, no loss/PLC
 * (lyra/lyra_decoder.cc:172-226,284-326): unpack -> DecodeToLossyFeatures -> generative model.
 * (Lost packets / DTX's empty packets on the device path: lyra_hip_decode_lossy_dev below.) */
int lyra_hip_decode(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B, const uint8_t* packets, int num_bits,
                    int16_t* pcm);

/* ---- device-pointer variants (benchmark / pipelines that keep data resident in HBM) ------------- */
int lyra_hip_extract_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B, const int16_t* d_pcm,
                         float* d_features);
int lyra_hip_rvq_encode_dev(lyra_hip_ctx* ctx, int B, const float* d_features, int num_bits, int32_t* d_indices);
int lyra_hip_rvq_decode_dev(lyra_hip_ctx* ctx, int B, const int32_t* d_indices, float* d_features);
int lyra_hip_generate_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B, const float* d_features,
                          int16_t* d_pcm);
int lyra_hip_logmel_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B, const int16_t* d_pcm, float* d_mel);
int lyra_hip_encode_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B, const int16_t* d_pcm, int num_bits,
                        uint8_t* d_packets);
int lyra_hip_decode_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B, const uint8_t* d_packets,
                        int num_bits, int16_t* d_pcm);
int lyra_hip_resample_dev(lyra_hip_ctx* ctx, int side, const int32_t* d_stream_ids, int B, const int16_t* d_in, int n_in,
                          int in_rate, int out_rate, int16_t* d_out);
int lyra_hip_comfort_noise_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B, const float* d_features,
                               int16_t* d_pcm);
int lyra_hip_noise_receive_dev(lyra_hip_ctx* ctx, int side, const int32_t* d_stream_ids, int B, const int16_t* d_pcm,
                               int32_t* d_is_noise);
/* (rows of d_packets that belong to noise hops are not written) */
int lyra_hip_encode_dtx_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B, const int16_t* d_pcm, int num_bits,
                            uint8_t* d_packets, int32_t* d_packet_bytes);

/* One hop at an EXTERNAL sample rate (8000 / 16000 / 32000 / 48000 Hz), ONE call per side -- the per-call form of what
 * LyraEncoder::Encode and LyraDecoder::DecodeSamples do around the codec for callers whose audio arrives hop by hop:
 *   encode_ext: the encoder's resampler (lyra_encoder.cc:119-122), with dtx != 0 the NoiseEstimator decision (:131-141; then
 *     d_packet_bytes [B] is required and lyra_hip_set_encoder_sample_rate(rate) must have been called), feature extractor,
 *     quantizer.  d_pcm_ext int16 [B][320 * rate / 16000].
 *   decode_ext: decode of a received hop into d_pcm16 [B][320], with estimate_noise != 0 the decoder-side NoiseEstimator
 *     (lyra_decoder.cc:304-311 -> d_is_noise [B]), the resampler to the external rate (:107-113 -> d_pcm_ext
 *     [B][320 * rate / 16000]; may be NULL at 16000).  The estimator and the resampler complete on the NOISE stream
 *     (lyra_hip_stream_noise / lyra_hip_stream_wait / lyra_hip_synchronize, as for lyra_hip_run_steps_dev).
 * Same results as lyra_hip_resample_dev + lyra_hip_encode[_dtx]_dev and lyra_hip_decode_dev + lyra_hip_noise_receive_dev +
 * lyra_hip_resample_dev.  The difference is what rule (2) of "Streams" counts: each of these is ONE call of its side, so
 * the next hop's encode overlaps this hop's decode; issued one by one, a hop makes two encode-side and up to three
 * decode-side calls and the next extractor / quantizer wait for this hop's decoder chain (4096 streams at 48 kHz: 10.4 M
 * frames/s call by call, 13.3 M through these two -- what lyra_hip_run_steps_dev reaches; profiles/r06_per_call.txt). */
int lyra_hip_encode_ext_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B, const int16_t* d_pcm_ext, int sample_rate_hz,
                            int num_bits, int dtx, uint8_t* d_packets, int32_t* d_packet_bytes);
int lyra_hip_decode_ext_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B, const uint8_t* d_packets, int num_bits,
                            int sample_rate_hz, int estimate_noise, int16_t* d_pcm16, int16_t* d_pcm_ext, int32_t* d_is_noise);

/* n_steps hops of B streams from ONE call (no host language in the loop): per hop what lyra_benchmark times
 * (lyra_benchmark_lib.cc:121-160) and what LyraEncoder::Encode / LyraDecoder::DecodeSamples run around it.  Step i
 * (absolute number first_step + i) reads input frame (first_step + i) % ring and uses buffer set (first_step + i) & 1
 * of every two-element array (the two-buffer rule above).  Same results, hop for hop, as the individual `_dev` calls
 * in the order resample -> encode[_dtx] -> decode | generate -> noise_receive -> resample. */
#define LYRA_HIP_STEP_ENCODE 1u         /* lyra_hip_encode_dev (lyra_encoder.cc:143-155) */
#define LYRA_HIP_STEP_DECODE 2u         /* lyra_hip_decode_dev on the packets of this step -- or, d_features != NULL,
                                           lyra_hip_generate_dev on those features (lyra_gan_model path) */
#define LYRA_HIP_STEP_DTX 4u            /* encode with enable_dtx: lyra_hip_encode_dtx_dev (lyra_encoder.cc:131-141) */
#define LYRA_HIP_STEP_DECODER_NOISE 8u  /* NoiseEstimator::ReceiveSamples on every decoded hop (lyra_decoder.cc:304-311) */
#define LYRA_HIP_STEP_PACKET_LOSS 16u   /* the decode leg is lyra_hip_decode_lossy_dev: row b of step `step` is received when
                                           d_received_ring[step % n_received_ring][b] != 0 (NULL: always) and, with
                                           ENCODE | DTX, the encoder's d_packet_bytes[set][b] != 0; the decoder-side
                                           estimator always runs, d_is_noise is optional.  Needs DECODE, no d_features.
                                           The three fields after d_ext_out are read only with this flag. */
#define LYRA_HIP_STEP_MIXED_BITRATE 32u /* per-stream bitrates: num_bits must be 0; step `step` takes the bit counts of row
                                           step % n_bits_ring of d_bits_ring.  The encode leg is lyra_hip_encode_mixed_dev
                                           (d_packet_bytes[2] required, DTX or not; packet rows LYRA_HIP_MAX_PACKET_BYTES
                                           apart).  DECODE needs PACKET_LOSS; its leg is lyra_hip_decode_lossy_mixed_dev on
                                           the encoder's d_packet_bytes[set] (with ENCODE) or, decode-only, on the sizes
                                           (bits + 7) / 8 of the same bits-ring row (d_packet_ring rows 23 bytes apart),
                                           combined with d_received_ring.  The two fields after d_is_comfort_noise are read
                                           only with this flag. */
#define LYRA_HIP_STEP_MIXED_RATE 64u    /* per-stream sample rates: d_rates [B] holds each stream's rate (constant over the steps
                                           of a call), external_rate must be 0; d_pcm_ring is [ring][B][LYRA_HIP_MAX_EXT_HOP],
                                           d_ext_out[2] are [B][LYRA_HIP_MAX_EXT_HOP].  The encode leg is
                                           lyra_hip_encode_rates_dev (d_packet_bytes[2] required, packet rows
                                           LYRA_HIP_MAX_PACKET_BYTES apart), the decode leg lyra_hip_decode_lossy_rates_dev
                                           (DECODE needs PACKET_LOSS).  With MIXED_BITRATE the bits of d_bits_ring, without it
                                           num_bits in every row.  The caller then passes the `steps` member of a
                                           lyra_hip_steps_rates (below): d_rates is read only with this flag.  NEVER set
                                           this flag on a plain lyra_hip_steps: the library would read the 8 bytes behind
                                           the struct as d_rates. */
typedef struct lyra_hip_steps {
  const int32_t* d_stream_ids;   /* [B] */
  int B;
  int num_bits;
  unsigned flags;                /* LYRA_HIP_STEP_* */
  long first_step;
  int n_steps;
  int ring;                      /* input frames in d_pcm_ring */
  const int16_t* d_pcm_ring;     /* [ring][B][320 * external_rate / 16000] */
  uint8_t* d_packets[2];         /* [B][num_bits / 8 rounded up] each */
  int32_t* d_packet_bytes[2];    /* [B] each (DTX) */
  int16_t* d_pcm_out[2];         /* [B][320] each: decoder output at 16 kHz */
  const float* d_features;       /* [n_features][B][64] or NULL: step `step` generates from frame step % n_features */
  int n_features;                /* frames in d_features (0 is read as 1) */
  const uint8_t* d_packet_ring;  /* DECODE without ENCODE: [n_packet_ring][B][bytes] received packets, or NULL (then
                                    d_packets[step & 1] is decoded as it stands) */
  int n_packet_ring;
  int32_t* d_is_noise;           /* [B] (DECODER_NOISE) */
  int external_rate;             /* 0 / 16000: none; 8000 / 32000 / 48000: the encoder's and the decoder's resampler
                                    (lyra_encoder.cc:119-122, lyra_decoder.cc:107-113) around the codec */
  int16_t* d_ext_out[2];         /* [B][320 * external_rate / 16000] each: decoder output at the external rate */
  /* LYRA_HIP_STEP_PACKET_LOSS only (appended: callers built against the struct without them keep working) */
  const uint8_t* d_received_ring;  /* [n_received_ring][B] 0 / 1, or NULL = all received */
  int n_received_ring;
  int32_t* d_is_comfort_noise;     /* [B] or NULL: is_comfort_noise() after the step's hop */
  /* LYRA_HIP_STEP_MIXED_BITRATE only (appended) */
  const int32_t* d_bits_ring;      /* [n_bits_ring][B] bit counts per step and stream: the caller's bitrate schedule */
  int n_bits_ring;
} lyra_hip_steps;
/* LYRA_HIP_STEP_MIXED_RATE: lyra_hip_steps with one field behind it.  lyra_hip_steps itself keeps its size and its last
 * field (callers and bindings built against it are untouched); in memory d_rates lies exactly where a field appended to
 * lyra_hip_steps would lie.  Call lyra_hip_run_steps_dev(ctx, &r.steps). */
typedef struct lyra_hip_steps_rates {
  lyra_hip_steps steps;
  const int32_t* d_rates;          /* [B] 8000 / 16000 / 32000 / 48000 per stream */
} lyra_hip_steps_rates;
int lyra_hip_run_steps_dev(lyra_hip_ctx* ctx, const lyra_hip_steps* steps);

/* ---- Packet loss on the device path: hop-synchronous receivers ---------------------------------------------------------
 * LyraDecoder::SetEncodedPacket (if a packet arrived) + DecodeSamples(one hop) for B streams (lyra_decoder.cc:172-373), the
 * case of decoder_main_lib.cc:95-135 and of a media server: on every 20 ms tick each stream receives one packet or none and
 * then decodes exactly one hop.  The reference's packet-loss concealment (ZeroFeatureEstimator features), the cosine
 * cross-fade to comfort noise after 80 ms of consecutive losses, the fade back when packets return and the decoder-side
 * NoiseEstimator fed with received hops only all run on the device; the per-stream state is three small integers kept in
 * the stream's comfort-noise slot (all zero after lyra_hip_create / lyra_hip_reset_streams = the reference's initial state).
 *   d_packet_bytes[b] == 0: no packet this hop (lost, or DTX's empty packet) -> concealment / comfort noise; otherwise it
 *   must equal the packet size of num_bits and row b of d_packets [B][num_bits / 8 rounded up] is read.  A value that is
 *   neither is treated as "no packet" and counted in a device error word (lyra_hip_decode_lossy_errors); it never faults.
 *   d_pcm16 [B][320]: the hop at 16 kHz; d_pcm_ext [B][sample_rate_hz / 50] (may be NULL at 16000): the same through the
 *   decoder's resampler; d_is_noise [B] (may be NULL): the decoder-side estimator's is_noise() after the tick (unchanged on
 *   ticks without a packet); d_is_comfort_noise [B] (may be NULL): LyraDecoder::is_comfort_noise() after the tick.
 * ONE decode-side call for rule (2) of "Streams".  Like lyra_hip_decode_ext_dev, its outputs -- d_pcm16 included, the mix
 * writes it -- complete on the NOISE stream (lyra_hip_stream_noise / lyra_hip_stream_wait / lyra_hip_synchronize).
 * Every stream of one call must be in the hop-synchronous regime: requests of up to one hop of any size are
 * lyra_hip_decode_samples_dev's (below), arbitrary DecodeSamples(n) requests BatchLyraDecoder's
 * (lyra_amd/host/lyra_batch_codec.cc).  Combinations:
 *   - LYRA_HIP_SUBBATCHES > 1: supported; the call is not split (it stands for every chunk, as small calls do);
 *   - lyra_hip_set_serial: supported; the call then also ends with its noise-stream half before the next encode-side call;
 *   - lyra_hip_decode_dev / lyra_hip_decode_ext_dev on the same stream: allowed -- they advance the generative model as a
 *     received hop would but neither read nor change the loss state or the comfort-noise generator; that is NOT what the
 *     reference computes for such a mix, so a stream should use one form between resets;
 *   - lyra_hip_comfort_noise[_dev] and the decoder twin use the same comfort-noise state: do not mix them with this call
 *     on one stream between resets. */
int lyra_hip_decode_lossy_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B, const uint8_t* d_packets,
                              const int32_t* d_packet_bytes, int num_bits, int sample_rate_hz, int16_t* d_pcm16,
                              int16_t* d_pcm_ext, int32_t* d_is_noise, int32_t* d_is_comfort_noise);
/* Number of d_packet_bytes values since context creation (or the last clear) that were neither 0 nor the packet size;
 * synchronises.  clear != 0 resets the count.  Negative: error. */
long lyra_hip_decode_lossy_errors(lyra_hip_ctx* ctx, int clear);

/* ---- Per-stream bitrates on the device path ------------------------------------------------------------------------------
 * Every LyraEncoder has a bitrate of its own that set_bitrate changes between hops (lyra_encoder.cc:158-166), and
 * LyraDecoder::SetEncodedPacket takes each packet's bitrate from its size (lyra_decoder.cc:172-179, lyra_config.h:99-106).
 * These two calls serve a batch whose streams run at different bitrates, changing on any hop, with ONE call per side.
 * Packet rows are LYRA_HIP_MAX_PACKET_BYTES apart in both directions; bytes past packet_bytes[b] in a row are never written
 * by the encoder and never read by the decoder.  Neither side keeps state that depends on the bitrate.
 *   encode_mixed: the per-row form of lyra_hip_encode_ext_dev (same resampler, DTX and rate rules; one encode-side call,
 *     packets written on the quantizer stream).  d_num_bits [B]: a multiple of 4 in 4..184 per row; row b's packet is what
 *     lyra_hip_encode_ext_dev makes for that stream at that bit count, byte for byte, packet_bytes[b] = num_bits[b] / 8
 *     rounded up (the last byte of an odd stage count carries a zero low nibble); a DTX noise hop gives 0.  An invalid
 *     d_num_bits[b] gives packet_bytes[b] = 0, leaves the row unwritten and is counted in a device error word
 *     (lyra_hip_encode_mixed_errors); the stream's encoder state advances as for a valid row.  d_packet_bytes is required.
 *   decode_lossy_mixed: lyra_hip_decode_lossy_dev with the packet size chosen per row as SetEncodedPacket does:
 *     d_packet_bytes[b] == 0: no packet; 8 / 15 / 23: received at 64 / 120 / 184 bits; any other value: no packet, counted
 *     in lyra_hip_decode_lossy_errors.  Everything else -- state, outputs, streams, combinations -- is lyra_hip_decode_lossy_dev's.
 * Both accept LYRA_HIP_SUBBATCHES > 1 (they are not split) and lyra_hip_set_serial.  In lyra_hip_run_steps_dev:
 * LYRA_HIP_STEP_MIXED_BITRATE. */
#define LYRA_HIP_MAX_PACKET_BYTES 23   /* packet row stride of the mixed calls: the 184-bit packet */
int lyra_hip_encode_mixed_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B, const int16_t* d_pcm_ext,
                              int sample_rate_hz, const int32_t* d_num_bits, int dtx,
                              uint8_t* d_packets /* [B][23] */, int32_t* d_packet_bytes /* [B], required */);
/* Number of invalid d_num_bits values since context creation (or the last clear); synchronises.  Negative: error. */
long lyra_hip_encode_mixed_errors(lyra_hip_ctx* ctx, int clear);
int lyra_hip_decode_lossy_mixed_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B,
                                    const uint8_t* d_packets /* [B][23] */, const int32_t* d_packet_bytes,
                                    int sample_rate_hz, int16_t* d_pcm16, int16_t* d_pcm_ext,
                                    int32_t* d_is_noise, int32_t* d_is_comfort_noise);

/* ---- Per-stream sample rates on the device path -----------------------------------------------------------------------
 * The sample rate is a property of each codec object (LyraEncoder::Create / LyraDecoder::Create: 8 / 16 / 32 / 48 kHz), so a
 * server has streams of all four rates in one tick.  These two calls serve such a batch with ONE call per side.
 * External-rate audio rows are LYRA_HIP_MAX_EXT_HOP samples apart in both directions; row b holds d_sample_rates[b] / 50
 * samples, the rest of the row is never read by the encoder and never written by the decoder.  Packet rows follow the
 * per-stream-bitrate conventions above.
 *   Row b of either call is, bit for bit, what the uniform call gives for that stream at that rate --
 *   lyra_hip_encode_mixed_dev(sample_rate_hz = rate[b]) after lyra_hip_set_encoder_sample_rate(rate[b]), and
 *   lyra_hip_decode_lossy_mixed_dev(sample_rate_hz = rate[b]) -- outputs and per-stream state alike: a stream may move
 *   between the per-row call and the uniform call at its rate from hop to hop without a reset.
 *   The per-row calls do NOT read lyra_hip_set_encoder_sample_rate's setting: with dtx != 0 each row's NoiseEstimator runs
 *   with the constants and the mel filterbank of its own rate (lyra_encoder.cc:82-85).
 *   Rows at 16000 have no resampler, as in the reference (lyra_encoder.cc:59, buffered_resampler.cc:123-126): the stream's
 *   resampler slot is neither read nor written; on the decode side the d_pcm_ext row receives the 320 samples of d_pcm16.
 *   A d_sample_rates[b] that is none of the four rates never faults and is counted in a device error word
 *   (lyra_hip_rates_errors).  Encoder: packet_bytes[b] = 0, the packet row is unwritten and NO state of that stream
 *   advances (resampler, estimator, extractor): the row is treated as absent from the hop.  Decoder: the tick runs as at
 *   16 kHz (d_pcm16, loss state, estimator as usual), the d_pcm_ext row is unwritten.
 *   A stream's rate belongs to the stream between resets.  Calling a stream with another rate without
 *   lyra_hip_reset_streams in between is a caller error with unspecified audio for that stream; it does not fault and does
 *   not disturb other rows.
 * Streams and ordering as the calls they generalise: one encode-side / one decode-side call for rule (2); packets complete
 * on the quantizer stream, decoder outputs on the noise stream; LYRA_HIP_SUBBATCHES > 1 accepted (not split);
 * lyra_hip_set_serial supported.  Null pointers (every argument but d_is_noise / d_is_comfort_noise is required) or B out of
 * range: LYRA_HIP_EINVAL, nothing enqueued.  In lyra_hip_run_steps_dev: LYRA_HIP_STEP_MIXED_RATE.
 * With DTX per stream as well, packed audio rows and a two-deep host-buffer form: lyra_hip_encode_streams.h; the decode
 * side with packed rows, an optional 16 kHz hop and the same host-buffer form: lyra_hip_decode_streams.h.  What a media
 * server does between the two -- every participant hears the sum of the others, decode, mix-minus and encode in one call:
 * lyra_hip_bridge.h; the same with only the few loudest talkers of each room in the mix, and who is speaking reported:
 * lyra_hip_speakers.h; and that with every distinct mix of a room encoded once and the packet shared by everyone who hears it:
 * lyra_hip_shared_bridge.h; a RECORDED meeting through the bridge, all ticks time-parallel in one call: lyra_hip_bridge_spans.h;
 * and one whose participants join, leave and move rooms while it runs, still in one call: lyra_hip_spans_meeting.h. */
#define LYRA_HIP_MAX_EXT_HOP 960   /* row stride, in samples, of external-rate audio in the calls below: the 48 kHz hop */
int lyra_hip_encode_rates_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B,
                              const int16_t* d_pcm_ext /* [B][960] */, const int32_t* d_sample_rates /* [B] */,
                              const int32_t* d_num_bits /* [B], as lyra_hip_encode_mixed_dev */, int dtx,
                              uint8_t* d_packets /* [B][23] */, int32_t* d_packet_bytes /* [B], required */);
int lyra_hip_decode_lossy_rates_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B,
                                    const uint8_t* d_packets /* [B][23] */, const int32_t* d_packet_bytes /* [B] */,
                                    const int32_t* d_sample_rates /* [B] */, int16_t* d_pcm16 /* [B][320] */,
                                    int16_t* d_pcm_ext /* [B][960], required */, int32_t* d_is_noise,
                                    int32_t* d_is_comfort_noise);
/* Number of invalid d_sample_rates values seen by either call since context creation (or the last clear); synchronises.
 * Negative: error. */
long lyra_hip_rates_errors(lyra_hip_ctx* ctx, int clear);

/* ---- Packet loss on the device path: any request size up to one hop -----------------------------------------------------
 * LyraDecoder::SetEncodedPacket (for the rows that got a packet) + DecodeSamples(num_samples) for B streams
 * (lyra_decoder.cc:172-373) when the receiver's request is NOT tied to the 20 ms hop: a WebRTC-style audio device that pulls
 * 10 ms while packets arrive every 20 ms, a jitter buffer that hands packets over early or late.  The reference's whole loop
 * -- GetNumSamplesToGenerate, concealment, the cross-fades to and from comfort noise, the generative model's feature FIFO,
 * the decoder-side NoiseEstimator fed with whole received hops -- runs on the device without any host decision or
 * synchronisation.  Per stream: seven integers in the comfort-noise slot (all zero after lyra_hip_create /
 * lyra_hip_reset_streams = the reference's initial state), plus the hop in progress of the generative model and of the
 * comfort-noise generator and the waiting feature vectors in arrays by stream id that the first call allocates.
 *   Packets: the row conventions of lyra_hip_decode_lossy_mixed_dev -- rows LYRA_HIP_MAX_PACKET_BYTES apart,
 *   d_packet_bytes[b] == 0: no packet in this call; 8 / 15 / 23: a packet at 64 / 120 / 184 bits; anything else: no packet,
 *   counted in lyra_hip_decode_samples_errors.  At most one packet per stream and call; a caller with two packets for a
 *   stream makes two calls, the second may have num_samples == 0 (SetEncodedPacket alone; d_pcm_ext may then be NULL).
 *   Request size: the same for every row of a call, free to change from call to call; 0 <= num_samples <=
 *   sample_rate_hz / 50 and num_samples * 16000 divisible by sample_rate_hz (any n at 8 and 16 kHz, even n at 32 kHz,
 *   multiples of 3 at 48 kHz; 10 ms qualifies at every rate), else LYRA_HIP_EINVAL and nothing is enqueued.  Under that rule
 *   BufferedResampler's leftover (buffered_resampler.cc:92-147) stays empty for ever.  Other sizes, and requests of up
 *   to four hops, are lyra_hip_decode_samples_any_dev's (lyra_hip_decode_samples_any.h).
 *   The feature FIFO holds LYRA_HIP_DECODE_SAMPLES_FIFO waiting vectors per stream (the reference's is unbounded): a packet
 *   that finds it full is NOT delivered -- the stream goes on as if the packet had never come -- and is counted in
 *   lyra_hip_decode_samples_errors.  A receiver that pulls audio at the rate packets arrive never holds more than 2.
 *   d_pcm_ext [B][num_samples] at sample_rate_hz (at 16000 the internal samples themselves); d_is_noise [B] (may be NULL):
 *   the decoder-side estimator's is_noise() after the call; d_is_comfort_noise [B] (may be NULL): is_comfort_noise().
 * ONE decode-side call for rule (2) of "Streams"; its outputs complete on the NOISE stream, as lyra_hip_decode_lossy_dev's
 * do.  LYRA_HIP_SUBBATCHES > 1 (the call is not split) and lyra_hip_set_serial are supported the same way.  For
 * num_samples = one hop the result is lyra_hip_decode_lossy_mixed_dev's bit for bit.  The state shares the comfort-noise
 * slot with lyra_hip_decode_lossy*_dev, the decoder twin and lyra_hip_comfort_noise[_dev] but is NOT theirs: do not mix
 * this call with any of them on one stream between resets.  lyra_hip_decode_dev / lyra_hip_decode_ext_dev on the same stream
 * advance the generative model without the loss state, as described for lyra_hip_decode_lossy_dev. */
#define LYRA_HIP_DECODE_SAMPLES_FIFO 4
int lyra_hip_decode_samples_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B,
                                const uint8_t* d_packets /* [B][23] */, const int32_t* d_packet_bytes /* [B] */,
                                int num_samples, int sample_rate_hz, int16_t* d_pcm_ext /* [B][num_samples] */,
                                int32_t* d_is_noise, int32_t* d_is_comfort_noise);
/* Invalid d_packet_bytes values plus packets that found the FIFO full since context creation (or the last clear);
 * synchronises.  clear != 0 resets the count.  Negative: error. */
long lyra_hip_decode_samples_errors(lyra_hip_ctx* ctx, int clear);
/* lyra_hip_decode_samples_dev with HOST buffers in two halves, up to two requests in flight (the form of
 * lyra_hip_decode_begin / _end; what DeviceLyraDecoder, lyra_amd/host/lyra_device_decoder.h, is built on).  begin() copies
 * ids [B], packets [B][23] and packet_bytes [B] into pinned staging at call time (the caller's arrays may be reused at once),
 * uploads them and enqueues the call; it does not synchronise.  end() delivers the OLDEST begun request's
 * [B][num_samples] samples into pcm (may be NULL for a request of 0 samples) and waits for that request only: the download
 * runs under the kernels of the request begun after it.  Errors of begin(): those of lyra_hip_decode_samples_dev, and
 * LYRA_HIP_EINVAL when two requests are already in flight. */
int lyra_hip_decode_samples_begin(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B, const uint8_t* packets /* [B][23] */,
                                  const int32_t* packet_bytes /* [B] */, int num_samples, int sample_rate_hz);
int lyra_hip_decode_samples_end(lyra_hip_ctx* ctx, int16_t* pcm /* [B][num_samples] */);

/* ---- Decoder twin: the device half of a batched LyraDecoder (lyra_amd/host/lyra_batch_codec.cc) ------------------------
 * LyraDecoder::DecodeSamplesInternal (lyra_decoder.cc:228-315) keeps per stream the conditioned hop of the generative
 * model and of the comfort-noise generator and hands out slices of them.  With these calls the two hops of every stream
 * stay on the device (arrays indexed by stream id); the caller runs the reference's per-stream state machine on integers
 * and describes each round of its loop.  All calls take HOST pointers, copy their arguments at call time, enqueue on
 * the decode-side stream and do NOT synchronise -- except lyra_hip_twin_fetch, which ends the request with one
 * device-to-host copy.  Per DecodeSamples call: packets + a few integers per stream up, the result down. */
/* RunConditioning for streams whose next hop comes from a received packet (SetEncodedPacket's DecodeToLossyFeatures +
 * AddFeatures happen here too, lyra_decoder.cc:198-206): packets [B][bytes of num_bits] -> generative-model hop of ids[b] */
int lyra_hip_twin_decode(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B, const uint8_t* packets, int num_bits);
/* ... from estimated features (packet loss concealment, ZeroFeatureEstimator::Estimate; lyra_decoder.cc:317-326) */
int lyra_hip_twin_conceal(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B);
/* comfort-noise hop of ids[b] from that stream's decoder-side noise estimate (lyra_decoder.cc:328-340) */
int lyra_hip_twin_comfort_noise(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B);
/* One pass of the reference's while loop for one stream: gen_n samples of the generative-model hop from gan_off and / or
 * cng_n samples of the comfort-noise hop from cng_off (equal when both are non-zero: cross-faded with fade_progress
 * `fade` stepping by fade_dir = +-1 per sample, MaybeOverlapAndInsert lyra_decoder.cc:342-373) to samples out_off.. of
 * row `id` of the request's output.  noise_row >= 0: the slice completes a received hop; its 320 samples become input
 * row noise_row of the lyra_hip_twin_noise call that follows (-1 otherwise). */
typedef struct lyra_hip_twin_slice {
  int32_t id, gan_off, gen_n, cng_off, cng_n, fade, fade_dir, out_off, noise_row;
} lyra_hip_twin_slice;
/* out_samples: internal-rate samples per stream of the whole request (the same in every call of one request) */
int lyra_hip_twin_assemble(lyra_hip_ctx* ctx, const lyra_hip_twin_slice* slices, int B, int out_samples);
/* NoiseEstimator::ReceiveSamples (lyra_decoder.cc:304-311) on the completed received hops marked by the preceding
 * lyra_hip_twin_assemble; stream_ids[r] = the stream whose slice carried noise_row r */
int lyra_hip_twin_noise(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B);
/* Ends the request: rows 0..num_streams-1 of the output, resampled from 16 kHz to out_rate when they differ (the
 * decoder-side resampler of streams 0..num_streams-1; any length, buffered_resampler.cc:120-128), into
 * out [num_streams][num_internal_samples * out_rate / 16000]; synchronises.  num_internal_samples == 0 just synchronises. */
int lyra_hip_twin_fetch(lyra_hip_ctx* ctx, int num_streams, int num_internal_samples, int out_rate, int16_t* out);

/* ---- Pipelined host-buffer calls (round 6) ----------------------------------------------------------------------------
 * Two-deep pipelined forms of the blocking host-buffer calls above, for a caller that feeds hop after hop: begin() copies
 * the small arrays (stream ids; the decoder's packets) into pinned slots of the context, uploads the audio STRAIGHT from the
 * caller's memory, waits on the host for that upload, enqueues the kernels and the download and returns; end() waits for the
 * OLDEST begun call and copies its result out.  At most two calls may be in flight; with begin(n + 1) issued before end(n)
 * the upload of hop n + 1 and the download of hop n run under the kernels (blocking calls idle the chain for both:
 * BatchLyraEncoder + BatchLyraDecoder on two host threads 7.8-8.3 M frames/s, pipelined: DESIGN.md 5).
 * The caller's buffers may be reused as soon as begin() / end() returns, pageable or pinned (hipHostMalloc,
 * hipHostRegister): begin() has read the small arrays on the host and has WAITED for the audio upload, in every branch;
 * end() has waited for its download (tests/test_gpu_pinned_buffers.py).  Which stream carries the upload: with another call
 * of the pipeline in flight, the context's noise stream (lyra_hip_stream_noise; it serves as the copy stream, no stream is
 * created for it), so that the copy runs under the older call's kernels; with none in flight, the encode-side stream itself.
 * The wait is for that stream: on a context that also runs decoder-side legs which complete on the noise stream
 * (lyra_hip_noise_receive_dev, lyra_hip_decode_ext_dev, lyra_hip_run_steps_dev with the estimator) begin() waits for those
 * kernels too -- keep an encoder pipeline and such decoder legs on contexts of their own if that matters.
 * Results are bit-identical to the blocking calls.  Do not mix blocking and pipelined calls of one kind on one context while
 * calls are in flight.
 *
 * lyra_hip_encode_begin: LyraEncoder::Encode for B streams (lyra/lyra_encoder.cc:113-156) -- pcm [B][sample_rate_hz / 50]
 *   at 8 / 16 / 32 / 48 kHz (the encoder's own resampler runs on the device, :119-122), dtx != 0 as lyra_hip_encode_dtx
 *   (call lyra_hip_set_encoder_sample_rate(sample_rate_hz) first).
 * lyra_hip_encode_end: packets [B][num_bits / 8 rounded up]; packet_bytes [B] may be NULL (required to tell DTX's empty
 *   packets apart). */
int lyra_hip_encode_begin(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B, const int16_t* pcm, int sample_rate_hz,
                          int num_bits, int dtx);
int lyra_hip_encode_end(lyra_hip_ctx* ctx, uint8_t* packets, int32_t* packet_bytes);
/* lyra_hip_decode in two halves: begin() takes packets [B][num_bits / 8 rounded up], end() delivers pcm [B][320] of the
 * oldest begun call (its download runs under a younger call's kernels). */
int lyra_hip_decode_begin(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B, const uint8_t* packets, int num_bits);
int lyra_hip_decode_end(lyra_hip_ctx* ctx, int16_t* pcm);
/* lyra_hip_twin_fetch in two halves ("Decoder twin" above): begin() ends the request being assembled -- its resampling and
 * its download are enqueued, the NEXT request's twin calls may follow at once --, end() waits for the oldest begun request
 * and copies its rows out (out may be NULL when that request had num_internal_samples == 0). */
int lyra_hip_twin_fetch_begin(lyra_hip_ctx* ctx, int num_streams, int num_internal_samples, int out_rate);
int lyra_hip_twin_fetch_end(lyra_hip_ctx* ctx, int16_t* out);

/* ---- Stream state as blobs: move live streams between ids, contexts, GPUs and processes ------------------------------------
 * A stream's whole codec state -- its slots in the 12 state regions plus what lyra_hip_decode_samples_dev keeps by stream id
 * (the waiting feature vectors and the two hops in progress) -- as ONE relocatable blob of lyra_hip_stream_blob_bytes()
 * bytes (a multiple of 256; format, header and the validation list: lyra_amd/csrc/stream_blob.h).  Row b of `blobs` is the
 * state of stream_ids[b]; rows are lyra_hip_stream_blob_bytes() apart.  A stream that is exported, imported elsewhere and
 * continued there produces, from the same inputs, bit for bit what it would have produced had it stayed -- comfort noise
 * included: the blob carries the stream's effective comfort-noise key (exporting context's seed ^ source id), and import
 * stores what makes the target slot keep that key under the target's seed and id.  Blobs of equal stream state are
 * byte-identical whichever context or id they came from; every freshly reset stream has the same blob.
 * Conventions:
 *   - CONTROL-PLANE calls with lyra_hip_reset_streams' ordering: the context is drained before and after, nothing is in
 *     flight while state is read or replaced, all four synchronise.  LYRA_HIP_EINVAL while a pipelined host request
 *     (lyra_hip_encode_begin, lyra_hip_decode_begin, lyra_hip_twin_fetch_begin, lyra_hip_decode_samples_begin without its
 *     _end, or a twin request being assembled) is outstanding.  There is no asynchronous form.
 *   - `_dev` forms: d_stream_ids and d_blobs are device pointers, d_blobs 16-byte aligned; a blob goes GPU to GPU without
 *     touching the host (copy it between devices yourself).  A row of id -1 is skipped; so is an id outside the context
 *     (counted by import; export leaves that blob row unwritten and counts nothing: clear d_blobs first if ids may be out
 *     of range).  The `_dev` forms cannot look at the ids: a call must not name a stream twice -- two rows of an import
 *     with the same target id race on its slots, as in every `_dev` call.  Host forms reject ids outside 0..max_streams-1 and duplicates, as every host form does.
 *   - `sides` of import: LYRA_HIP_STATE_ENCODER writes the encoder's regions only (the three encoder stages, the DTX noise
 *     estimator, the input resampler), LYRA_HIP_STATE_DECODER the decoder's (the three decoder stages, log-mel history,
 *     decoder-side noise estimator, output resampler, comfort-noise generator with the loss state machines, and the
 *     decode-samples arrays, which are allocated as the first lyra_hip_decode_samples_dev call would).  The other side of
 *     the target stream is left as it is.  Export always writes both.
 *   - A blob is untrusted.  Import checks the header against its own constants and every integer of the payload that a
 *     kernel forms an address or a trip count from against its domain, BEFORE it writes.  The `_dev` form refuses row by
 *     row on the device: a refused row leaves its target stream untouched, adds one to lyra_hip_import_errors, and the other
 *     rows of the call are imported.  The host form validates every row on the host first and returns LYRA_HIP_EINVAL with
 *     nothing enqueued and nothing changed if any row fails.
 *   - Caller duties: a stream's sample rate travels with it (the rate belongs to the stream, see
 *     lyra_hip_encode_rates_dev), as does the DTX encoder's lyra_hip_set_encoder_sample_rate.  Source and target context
 *     must have the same requant mode; a blob from another mode, model version or state layout is refused, not converted.
 *   - Not in a blob: the decoder twin's by-id hops (BatchLyraDecoder keeps its per-stream state on the host). */
#define LYRA_HIP_STATE_ENCODER 1u
#define LYRA_HIP_STATE_DECODER 2u
size_t lyra_hip_stream_blob_bytes(void);
int lyra_hip_export_streams_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B, uint8_t* d_blobs);
int lyra_hip_import_streams_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B, const uint8_t* d_blobs, unsigned sides);
int lyra_hip_export_streams(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B, uint8_t* blobs);
int lyra_hip_import_streams(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B, const uint8_t* blobs, unsigned sides);
/* Blob rows lyra_hip_import_streams_dev refused since context creation (or the last clear); synchronises.  clear != 0
 * resets the count.  Negative: error. */
long lyra_hip_import_errors(lyra_hip_ctx* ctx, int clear);

/* ---- Time-parallel spans: one long recording through the batched kernels ------------------------------------------------------
 * The whole encoder and decoder state is convolution history, so a stream that starts from the reset state
 * lyra_hip_span_warmup_frames(side) hops early holds, after them, exactly the state of the stream that ran from the start
 * (derivation from the graphs' kernel sizes, strides and dilations: DESIGN.md 4.5, lyra_amd/csrc/spans_plan.h).  These calls
 * cut long spans into chunks, run chunk 0 on the span's own stream and the others on scratch streams ("lanes") behind a
 * discarded warm-up, all chunks advancing together through the batched stage kernels, and hand the last chunk's state back:
 * packets, PCM and the span stream's state afterwards are the sequential result BIT FOR BIT, at batch throughput, for
 * (L + W) / L times the work with chunks of L hops.
 *   A span is n_frames consecutive hops of stream stream_id that lie at frame first_frame of the two FRAME-MAJOR buffers
 *   (PCM [frames][320] int16, 16-byte aligned; packets [frames][num_bits / 8 rounded up]); frames outside every span are
 *   neither read nor written.  A span CONTINUES from its stream's live state (for a fresh stream it is the whole file) and
 *   leaves the stream as the hop-by-hop calls would: lyra_hip_export_streams gives the same bytes, hop-by-hop calls may follow.
 *   Only the encoder's (encode_spans) or the decoder's (decode_spans) three stage regions of the stream change.
 *   Lanes are streams of the same context that the caller lends for the call; whatever they held is lost: their encoder-side
 *   (encode_spans) or decoder-side (decode_spans) stage state is the reset state when the call's work is done.
 *   n_lanes == 0, or spans too short to cut, run sequentially on the spans' own ids.
 *   Span ids and lane ids must be valid, distinct and disjoint and the spans' frame ranges non-negative and disjoint, else
 *   LYRA_HIP_EINVAL with nothing enqueued.  spans and lane_ids are HOST arrays in every form, copied at call time.
 *   `_dev` forms enqueue and do not synchronise (a call that follows another span call of its side first waits until that
 *   call's plan upload has run); each is ONE call of its side for rules (1) to (3) of "Streams" and runs on
 *   lyra_hip_stream() / lyra_hip_stream_decode() -- the packets too, the quantizer stream is not used.  The host-buffer forms
 *   stage frames 0 .. the last span's end, run, synchronise and write the spans' frames of the output.
 *   Sample rates: the `_ext` forms take the PCM at sample_rate_hz = 8000 / 16000 / 32000 / 48000, rows of sample_rate_hz / 50
 *   samples (160 / 320 / 640 / 960: every row a multiple of 16 bytes), ONE rate per call.  The resampler's state is its last 34
 *   input samples and a decimation phase -- history again, and so short that it needs no lanes: one launch resamples every
 *   frame of every span, in front of the steps (encode) or behind them (decode); frame 0 of a span continues from the span
 *   stream's resampler slot and leaves in it what the hop-by-hop calls would.  Packets, external-rate PCM and stream state
 *   are BIT FOR BIT those of lyra_hip_resample[_dev](ENCODER) + lyra_hip_encode[_dev] per hop (lyra_hip_encode_ext_dev
 *   without DTX) and of lyra_hip_decode[_dev] + lyra_hip_resample[_dev](DECODER) per hop, whether the span continues a live
 *   stream or hop-by-hop calls follow it.  Besides the three stage regions only the resampler slot of the span streams' side
 *   changes; the lanes' resampler slots are not touched.
 *   d_pcm16 [frames][320] is the caller's 16 kHz workspace (16-byte aligned; the `_dev` forms allocate nothing, the host forms
 *   keep it next to their staging buffers): after encode it holds the resampled audio of the spans' frames, after decode the
 *   16 kHz output, as in lyra_hip_decode_ext_dev; other rows are not touched.  At 16000 the call is the plain span call on the
 *   external-rate buffer, d_pcm16 may be NULL and no resampler slot is read or written.  Any other rate, a null or misaligned
 *   buffer or anything the planner refuses: LYRA_HIP_EINVAL with nothing enqueued.
 *   Each `_ext` call is ONE call of its side as above and the resampler pass runs on the side's own stream inside it:
 *   UNLIKE lyra_hip_decode_ext_dev, whose external-rate output completes on the noise stream, everything a
 *   lyra_hip_decode_spans_ext_dev call writes completes on lyra_hip_stream_decode().
 *   DTX: lyra_hip_encode_spans_dtx[_dev] is LyraEncoder::Encode with enable_dtx over the spans.  The NoiseEstimator is a true
 *   recurrence, not history -- but it reads the 16 kHz input audio alone, never encoder state (lyra_encoder.cc:113-156), so its
 *   decisions are computed for all frames in front of the steps: [the resampler pass at 8 / 32 / 48 kHz,] the estimator's
 *   log-mel of every frame in one launch, then one wavefront per span walking the recurrence frame by frame.  Under DTX the
 *   encoder does not advance on noise hops (lyra_hip_encode_dtx): what it sees is the subsequence of non-noise hops, again a
 *   stream whose state is convolution history, so the planner, lanes, warm-up and hand-over apply unchanged to that compacted
 *   frame list (warm-up counted in non-noise hops).
 *   Per span frame, packet_bytes (0 = empty packet, else num_bits / 8 rounded up) and the packet row are BIT FOR BIT what
 *   lyra_hip_resample(ENCODER) + lyra_hip_encode_dtx per hop give; in the host form the rows of noise frames are left zero, in
 *   the `_dev` form they are not written.  Afterwards the span streams' encoder stages, encoder-side estimator slot and
 *   resampler slot are what those calls leave (lyra_hip_export_streams returns the same bytes); a span continues a live stream
 *   and may be continued hop by hop.  Lanes lend encoder stage state only and come back reset; their estimator and resampler
 *   slots are not touched.  Frames outside every span are untouched in every buffer.  A span with no non-noise frame runs no
 *   chunk and leaves the encoder stage regions untouched.  d_pcm16 as in the `_ext` forms (may be NULL at 16000).
 *   sample_rate_hz must equal the context's lyra_hip_set_encoder_sample_rate (the rule of lyra_hip_encode_ext_dev with dtx);
 *   d_packet_bytes is required.  That, ids, lanes, frame ranges (the planner's rules on the spans as given), pointers,
 *   alignment and the bit count are checked before the first kernel is enqueued: LYRA_HIP_EINVAL leaves the estimator
 *   untouched.  All scratch is sized for the worst case (every frame non-noise) up front.
 *   The call is ONE encode-side call on lyra_hip_stream().  UNLIKE the other `_dev` span calls it BLOCKS THE HOST ONCE, until
 *   the scan has finished, because the plan depends on the decisions; everything behind that point is enqueued without
 *   synchronising.  lyra_hip_set_serial is supported.
 *   lyra_hip_noise_spans[_dev] is the estimator alone, NoiseEstimator::ReceiveSamples over every frame of every span of the
 *   16 kHz buffer (16-byte aligned): is_noise[frame] is what lyra_hip_noise_receive returns for that hop and the stream's
 *   estimator slot afterwards what the hop-by-hop calls leave.  Side ENCODER uses the constants and filterbank of
 *   lyra_hip_set_encoder_sample_rate and is an encode-side call, side DECODER those of 16 kHz and is a decode-side call on
 *   lyra_hip_stream_decode().  No lanes; the `_dev` form does not synchronise.
 *   Packet loss: lyra_hip_decode_spans_lossy[_dev] is lyra_hip_decode_lossy_dev(sample_rate_hz) -- SetEncodedPacket when a packet
 *   arrived + DecodeSamples(one hop), with concealment, comfort noise and cross-fades -- over the spans.  packet_bytes is a HOST
 *   array like spans and lane_ids, [frames], 0 = no packet (lost, or DTX's empty packet), else num_bits / 8 rounded up: a
 *   receiver knows which packets arrived.  The loss state machine depends on that pattern and on the stream's control word
 *   alone, so every tick's legs are planned on the host (lyra_hip_spans_lossy_plan): the generative model advances on its ticks
 *   only, from the packet or from zero features -- convolution history again, so planner, lanes, warm-up and hand-over apply to
 *   the compacted list of those ticks; the decoder-side NoiseEstimator is a recurrence over the generative hops of the received
 *   ticks (one log-mel launch, one wavefront per span); a comfort-noise tick reads the estimate as it stood after the received
 *   frames in front of it, which the scan leaves as snapshots, and its phases are counter-based, so only the overlap-add is
 *   ordered; mix and resampler are passes over all frames.
 *   Per span frame d_pcm16 [frames][320] (required), d_pcm_ext [frames][rate / 50] (rate != 16000), d_is_noise (unchanged across
 *   ticks without a packet) and d_is_comfort_noise (both optional) are BIT FOR BIT what lyra_hip_decode_lossy_dev gives hop by
 *   hop on that stream.  Afterwards the span streams' three decoder stage regions, decoder-side estimator slot (log-mel history
 *   included), comfort-noise slot (hop counter, accumulator, control word) and output resampler slot are what those calls
 *   leave: lyra_hip_export_streams returns the same bytes.  A span continues a live stream, mid-burst included, and
 *   lyra_hip_decode_lossy*_dev calls may follow it.  Lanes lend decoder stage state only and come back reset; their other
 *   slots are untouched.  Frames outside every span are untouched in every buffer; a span with no generative tick runs no chunk.
 *   A packet_bytes value that is neither 0 nor the size of num_bits, bad ids, lanes, ranges, pointers, alignment or rate and
 *   anything the planner refuses: LYRA_HIP_EINVAL with nothing enqueued and no state changed.
 *   The call is ONE decode-side call and everything it writes completes on lyra_hip_stream_decode() (UNLIKE the hop-by-hop
 *   call, whose outputs complete on the noise stream).  It BLOCKS THE HOST ONCE, at its start, to read the span streams' 4-byte
 *   control words; everything after that is enqueued without synchronising.  lyra_hip_set_serial is supported.  The state is the
 *   hop-synchronous call's: the "do not mix" rules of lyra_hip_decode_lossy_dev hold, lyra_hip_decode_samples_dev keeps its own.
 *   Per-frame bitrates (set_bitrate between hops; a packet size per frame): lyra_hip_spans_mixed.h, which includes this header.
 *   Per-span sample rates (recordings at 8, 16, 32 and 48 kHz in one call): lyra_hip_spans_rates.h, which includes that one.
 * Out of scope: request sizes other than one hop on spans.
 * LYRA_HIP_SUBBATCHES > 1 is accepted (the calls are not split). */
typedef struct lyra_hip_span { int32_t stream_id; int64_t first_frame; int64_t n_frames; } lyra_hip_span;
/* warm-up hops of side LYRA_HIP_SIDE_ENCODER / LYRA_HIP_SIDE_DECODER (25 / 25); LYRA_HIP_EINVAL for any other side */
int lyra_hip_span_warmup_frames(int side);
int lyra_hip_encode_spans_dev(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                              const int16_t* d_pcm /* [frames][320] */, int num_bits, uint8_t* d_packets /* [frames][bytes] */);
int lyra_hip_decode_spans_dev(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                              const uint8_t* d_packets /* [frames][bytes] */, int num_bits, int16_t* d_pcm /* [frames][320] */);
int lyra_hip_encode_spans(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                          const int16_t* pcm, int num_bits, uint8_t* packets);
int lyra_hip_decode_spans(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                          const uint8_t* packets, int num_bits, int16_t* pcm);
int lyra_hip_encode_spans_ext_dev(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                  const int16_t* d_pcm_ext /* [frames][rate / 50] */, int sample_rate_hz,
                                  int16_t* d_pcm16 /* [frames][320] workspace */, int num_bits, uint8_t* d_packets);
int lyra_hip_decode_spans_ext_dev(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                  const uint8_t* d_packets, int num_bits, int sample_rate_hz,
                                  int16_t* d_pcm16 /* [frames][320] */, int16_t* d_pcm_ext /* [frames][rate / 50] */);
int lyra_hip_encode_spans_ext(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                              const int16_t* pcm_ext, int sample_rate_hz, int num_bits, uint8_t* packets);
int lyra_hip_decode_spans_ext(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                              const uint8_t* packets, int num_bits, int sample_rate_hz, int16_t* pcm_ext);
int lyra_hip_encode_spans_dtx_dev(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                  const int16_t* d_pcm_ext /* [frames][rate / 50] */, int sample_rate_hz,
                                  int16_t* d_pcm16 /* [frames][320] workspace; may be NULL at 16000 */, int num_bits,
                                  uint8_t* d_packets /* [frames][bytes] */, int32_t* d_packet_bytes /* [frames], required */);
int lyra_hip_encode_spans_dtx(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                              const int16_t* pcm_ext, int sample_rate_hz, int num_bits, uint8_t* packets, int32_t* packet_bytes);
int lyra_hip_noise_spans_dev(lyra_hip_ctx* ctx, int side, const lyra_hip_span* spans, int n_spans,
                             const int16_t* d_pcm16 /* [frames][320] */, int32_t* d_is_noise /* [frames] */);
int lyra_hip_noise_spans(lyra_hip_ctx* ctx, int side, const lyra_hip_span* spans, int n_spans, const int16_t* pcm16,
                         int32_t* is_noise);
int lyra_hip_decode_spans_lossy_dev(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                    const uint8_t* d_packets /* [frames][bytes of num_bits] */,
                                    const int32_t* packet_bytes /* HOST [frames]: 0 = no packet, else the size of num_bits */,
                                    int num_bits, int sample_rate_hz, int16_t* d_pcm16 /* [frames][320], required */,
                                    int16_t* d_pcm_ext /* [frames][rate / 50]; may be NULL at 16000 */,
                                    int32_t* d_is_noise /* [frames] or NULL */, int32_t* d_is_comfort_noise /* [frames] or NULL */);
int lyra_hip_decode_spans_lossy(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                const uint8_t* packets, const int32_t* packet_bytes, int num_bits, int sample_rate_hz,
                                int16_t* pcm16, int16_t* pcm_ext, int32_t* is_noise, int32_t* is_comfort_noise);
/* The planner of the four calls, a pure function (no context, no device).  Chunk r is row r of the call's batch: it runs on
 * stream_id for n_warmup + n_frames steps; step i reads buffer frame first_frame - n_warmup + i and from step n_warmup on
 * writes its output there.  Chunk 0 of a span runs on the span's own stream with no warm-up; the others on lanes, behind
 * n_warmup = lyra_hip_span_warmup_frames(side) hops of the span's own earlier frames.  Order: the spans' own chunks by falling
 * step count, then the lane chunks by falling step count, so the lanes that run at step i are a prefix of the lane rows.
 * phase_offset (lanes): frames of the span in front of the chunk's first replayed hop, mod 18 -- the lane's ring phases start
 * at the span stream's plus this, so the state that the last chunk (last = 1) hands over has the sequential stream's.
 * What it minimises: the number of steps (about the longest chunk + warm-up), see lyra_amd/csrc/spans_plan.h.
 * Returns the number of chunks written (<= n_spans + n_lanes; spans of no frames have none), *n_steps = steps of the call;
 * LYRA_HIP_EINVAL for ids outside 0..max_streams-1 or named twice, overlapping frame ranges, negative values, cap too small. */
typedef struct lyra_hip_span_chunk {
  int32_t stream_id, span;
  int64_t first_frame;
  int32_t n_frames, n_warmup, phase_offset, last;
} lyra_hip_span_chunk;
int lyra_hip_spans_plan(int side, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes, int max_streams,
                        lyra_hip_span_chunk* chunks, int cap, int* n_steps);
/* The planner of lyra_hip_decode_spans_lossy, a pure function too (lyra_amd/csrc/spans_lossy_plan.h).  ctl_in[s]: the control
 * word of span s's stream on entry (0 for a fresh stream; lyra_amd/csrc/lossy_plan.h).  Per span, counts[s]; the lists of all
 * spans lie span after span, dense, in arrays of (sum of n_frames) entries each, any of which may be NULL:
 *   gen_frames / gen_received  buffer frames of the ticks that run the generative model, 1 = from the packet, 0 = concealed
 *   rx_frames                  buffer frames of the received ticks (the estimator's input, in order)
 *   cng_frames / cng_versions  buffer frames of the comfort-noise ticks and the number of received frames of the span in front of
 *                              each: the version of the estimate it reads (0 = the estimate on entry)
 *   versions                   those versions, rising, each once: what the scan snapshots
 *   info                       lossy_info per frame of the span
 * chunks / n_steps: lyra_hip_spans_plan(DECODER) on the compacted spans (stream_id, start in gen_frames, n_gen): first_frame
 * counts in gen_frames.  Returns the number of chunks; LYRA_HIP_EINVAL for what lyra_hip_spans_plan refuses, a packet_bytes
 * value that is neither 0 nor packet_size, cap too small. */
typedef struct lyra_hip_span_lossy_counts {
  int64_t n_gen, n_received, n_cng, n_versions;
  uint32_t ctl_out; /* the control word after the span */
  int32_t reserved;
} lyra_hip_span_lossy_counts;
int lyra_hip_spans_lossy_plan(const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes, int max_streams,
                              const int32_t* packet_bytes, int packet_size, const uint32_t* ctl_in,
                              lyra_hip_span_lossy_counts* counts, int64_t* gen_frames, uint8_t* gen_received, int64_t* rx_frames,
                              int64_t* cng_frames, int32_t* cng_versions, int32_t* versions, int32_t* info,
                              lyra_hip_span_chunk* chunks, int cap, int* n_steps);

/* The context's FOUR HIP streams (hipStream_t as void*), for event timing / ordering by the caller: encode side, decode
 * side, the quantizer stream of lyra_hip_encode_dev / lyra_hip_encode_dtx_dev, and the noise stream.
 *  - The packets of the two encode calls are written on the QUANTIZER stream: lyra_hip_stream() does not cover them (it
 *    covers every other encode-side output).
 *  - The decoder-side lyra_hip_noise_receive_dev (d_is_noise and the estimator's state) and, inside
 *    lyra_hip_run_steps_dev at an external rate, the output resampler (d_ext_out) complete on the NOISE stream: an event
 *    recorded on lyra_hip_stream_decode() after those calls does NOT cover them -- use lyra_hip_stream_noise(),
 *    lyra_hip_stream_wait() or lyra_hip_synchronize().
 * lyra_hip_synchronize() waits for all four; lyra_hip_stream_wait() orders a caller's stream behind all four. */
void* lyra_hip_stream(lyra_hip_ctx* ctx);
void* lyra_hip_stream_decode(lyra_hip_ctx* ctx);
void* lyra_hip_stream_quantizer(lyra_hip_ctx* ctx);
void* lyra_hip_stream_noise(lyra_hip_ctx* ctx);
int lyra_hip_synchronize(lyra_hip_ctx* ctx);
/* Ordering against a caller-owned HIP stream (hipStream_t as void*, NULL = the null stream); see "Streams". */
int lyra_hip_wait_for_stream(lyra_hip_ctx* ctx, void* caller_stream);
int lyra_hip_stream_wait(lyra_hip_ctx* ctx, void* caller_stream);
/* on != 0: encode-side calls also wait for the MOST RECENT decode-side call, i.e. the library streams run
 * strictly in call order (one buffer set suffices; per-kernel timings are free of cross-stream contention). */
int lyra_hip_set_serial(lyra_hip_ctx* ctx, int on);
/* Stream priorities of the encode-side / decode-side / quantizer streams, 0 (lowest) .. 2 (highest); default 0, 0, 2.  The
 * context is drained and the three streams are created anew (HIP fixes a priority at creation).  A context that serves
 * BLOCKING decode calls beside another context's encoder (BatchLyraDecoder next to BatchLyraEncoder) wants its decode side
 * first -- (0, 2, 2), the schedule of rounds 2-3: the decode kernels win the arbitration and the call returns sooner
 * (7.2 M vs 6.4 M frames/s on two host threads); the `_dev` pipeline of one context wants the default (see
 * LYRA_HIP_PRIO under lyra_hip_create).  CU-masked streams (contexts of <= 1024 streams) have no priority.  Handles obtained
 * earlier from lyra_hip_stream() / lyra_hip_stream_decode() / lyra_hip_stream_quantizer() are invalid afterwards. */
int lyra_hip_set_stream_priorities(lyra_hip_ctx* ctx, int encode_side, int decode_side, int quantizer);

/* Per-stream state footprint in HBM (bytes) and the context's stream capacity. */
size_t lyra_hip_state_bytes_per_stream(void);
int lyra_hip_max_streams(const lyra_hip_ctx* ctx);

/* Measurement hook (bench.py): launches of every kernel whose bit is set in `kernel_mask` (bit i = kernel i of
 * lyra_hip_profile_kernel_name) are bracketed by HIP events recorded on the context's stream; 0 disables.
 * profile_read() synchronises, returns per-kernel total milliseconds and launch counts since the previous read
 * (arrays of lyra_hip_profile_kernel_count() entries) and clears them. */
int lyra_hip_profile_enable(lyra_hip_ctx* ctx, unsigned kernel_mask);
/* Bracket only every `every`-th launch of an enabled kernel (default 1): an event record is a packet of its own in the
 * stream (~5 us of bubble on MI355X), so timing every launch of a kernel inside a throughput measurement slows the
 * measured pipeline itself. */
int lyra_hip_profile_sample(lyra_hip_ctx* ctx, int every);
int lyra_hip_profile_kernel_count(void);
const char* lyra_hip_profile_kernel_name(int i);
int lyra_hip_profile_read(lyra_hip_ctx* ctx, double* total_ms, long* launches);
/* start / end (ms, relative to the first recorded span's start) of every span recorded since the last read; call
 * BEFORE lyra_hip_profile_read.  Returns the number of spans written (<= cap) or a negative error. */
int lyra_hip_profile_timeline(lyra_hip_ctx* ctx, int cap, int* kernel_ids, float* start_ms, float* end_ms);

/* Test hook: copies stage-boundary activations of the LAST extract/generate call (device scratch) to host.
 * which: 0 enc stage0 out [B][4][128], 1 enc stage1 out [B][2][256], 2 enc int8 codes [B][64] (as f32),
 *        3 dec head out [B][4][128], 4 dec stage1 out [B][20][64],
 *        5 the quantizer's exact-chain counters since creation (2 floats; lyra_hip_encode_mixed_dev adds the stages
 *        a 16-frame tile runs past a shorter frame's own count).  Channel order is the library's
 *        internal one; returns the number of floats written or a negative error. */
long lyra_hip_debug_read(lyra_hip_ctx* ctx, int which, float* host_out, long capacity);

#ifdef __cplusplus
}
#endif
#endif /* LYRA_HIP_H_ */
