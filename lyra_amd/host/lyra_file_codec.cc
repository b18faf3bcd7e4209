// lyra_file_codec.cc -- see lyra_file_codec.h.  Plain C++17 over the C ABI (include/lyra_hip.h); no HIP here.
#include "lyra_file_codec.h"

#include <algorithm>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>

#include "../../include/lyra_hip.h"
#include "../../include/lyra_hip_spans_mixed.h"
#include "../../include/lyra_hip_spans_packed.h"
#include "glog/logging.h"
#include "lyra_batch_codec.h"

// The span calls are bound weakly: this file also links against builds of the C ABI that predate them (an older
// liblyra_hip.so, the CPU stand-in of the host-logic tests), where the time-parallel functions report that and fail --
// the `_ext` pair on its own, so that a library with the plain span calls alone still serves 16 kHz.
#pragma weak lyra_hip_encode_spans
#pragma weak lyra_hip_decode_spans
#pragma weak lyra_hip_span_warmup_frames
#pragma weak lyra_hip_encode_spans_ext
#pragma weak lyra_hip_decode_spans_ext
#pragma weak lyra_hip_encode_spans_dtx
#pragma weak lyra_hip_decode_spans_lossy
#pragma weak lyra_hip_encode_spans_mixed
#pragma weak lyra_hip_decode_spans_lossy_mixed
#pragma weak lyra_hip_encode_spans_packed
#pragma weak lyra_hip_decode_spans_lossy_packed
#pragma weak lyra_hip_decode_spans_packed

namespace chromemedia {
namespace codec {
namespace {

struct Ctx {  // RAII around one GPU context
  lyra_hip_ctx* c = nullptr;
  ~Ctx() { if (c) lyra_hip_destroy(c); }
  // what: "encoder" / "decoder", for the log line
  bool Create(const ghc::filesystem::path& model_path, int device, int max_streams, const char* what) {
    if (lyra_hip_create(model_path.string().c_str(), device, max_streams, LYRA_HIP_REQUANT_DEFAULT, &c) == 0) return true;
    LOG(ERROR) << "Could not create lyra " << what << ": " << lyra_hip_last_error(nullptr);
    return false;
  }
};

bool CheckScope(int num_channels, int sample_rate_hz, bool enable_preprocessing, bool enable_dtx) {
  if (num_channels != 1) {
    LOG(ERROR) << "Number of channels " << num_channels << " is not supported by codec. It needs to be 1.";
    return false;
  }
  if (sample_rate_hz != 8000 && sample_rate_hz != 16000 && sample_rate_hz != 32000 && sample_rate_hz != 48000) {
    LOG(ERROR) << "Sample rate " << sample_rate_hz << " Hz is not supported by codec. It needs to be 8000, 16000, 32000 or 48000.";
    return false;
  }
  if (enable_preprocessing) {
    LOG(ERROR) << "Preprocessing is not part of this build.";
    return false;
  }
  (void)enable_dtx;   // LyraEncoder's DTX: lyra_hip_encode_dtx per hop / lyra_hip_encode_spans_dtx
  return true;
}

// num_bits of the bitrate whose packets are packet_size bytes, -1 (logged): none
int NumBitsOfPacketSize(int packet_size) {
  for (int br : {3200, 6000, 9200})
    if (BatchBitrateToPacketSize(br) == packet_size) return BatchBitrateToNumQuantizedBits(br);
  LOG(ERROR) << "The packet size (" << packet_size << " bytes) is not supported.";
  return -1;
}

bool WholePackets(const std::vector<std::vector<uint8_t>>& packet_streams, int packet_size) {
  for (const auto& p : packet_streams)
    if (p.size() % packet_size != 0) { LOG(ERROR) << "Encoded stream is not a whole number of packets."; return false; }
  return true;
}

uint32_t Rd32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
uint16_t Rd16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
void Wr32(std::vector<uint8_t>* v, uint32_t x) { for (int i = 0; i < 4; ++i) v->push_back((x >> (8 * i)) & 255); }
void Wr16(std::vector<uint8_t>* v, uint16_t x) { v->push_back(x & 255); v->push_back(x >> 8); }

}  // namespace

bool ReadWav16(const ghc::filesystem::path& path, std::vector<int16_t>* samples, int* num_channels,
               int* sample_rate_hz) {
  std::ifstream in(path.string(), std::ios::binary);
  if (!in.is_open()) { LOG(ERROR) << "Could not open " << path.string(); return false; }
  std::vector<uint8_t> b((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  if (b.size() < 12 || std::memcmp(b.data(), "RIFF", 4) != 0 || std::memcmp(b.data() + 8, "WAVE", 4) != 0) {
    LOG(ERROR) << path.string() << " is not a RIFF/WAVE file.";
    return false;
  }
  bool have_fmt = false;
  size_t pos = 12;
  while (pos + 8 <= b.size()) {
    const uint32_t len = Rd32(&b[pos + 4]);
    const uint8_t* body = &b[pos + 8];
    if (std::memcmp(&b[pos], "fmt ", 4) == 0 && len >= 16 && pos + 8 + 16 <= b.size()) {
      const int format = Rd16(body), bits = Rd16(body + 14);
      *num_channels = Rd16(body + 2);
      *sample_rate_hz = (int)Rd32(body + 4);
      if (format != 1 || bits != 16) { LOG(ERROR) << path.string() << ": only 16-bit PCM is supported."; return false; }
      have_fmt = true;
    } else if (std::memcmp(&b[pos], "data", 4) == 0) {
      if (!have_fmt) { LOG(ERROR) << path.string() << ": data chunk before fmt chunk."; return false; }
      const size_t n = std::min<size_t>(len, b.size() - (pos + 8)) / 2;
      samples->resize(n);
      std::memcpy(samples->data(), body, n * 2);
      return true;
    }
    pos += 8 + (size_t)len + (len & 1);
  }
  LOG(ERROR) << path.string() << ": no data chunk.";
  return false;
}

bool WriteWav16(const ghc::filesystem::path& path, const std::vector<int16_t>& samples, int num_channels,
                int sample_rate_hz) {
  std::vector<uint8_t> h;
  const uint32_t data_bytes = (uint32_t)(samples.size() * 2);
  h.insert(h.end(), {'R', 'I', 'F', 'F'}); Wr32(&h, 36 + data_bytes);
  h.insert(h.end(), {'W', 'A', 'V', 'E', 'f', 'm', 't', ' '}); Wr32(&h, 16);
  Wr16(&h, 1); Wr16(&h, (uint16_t)num_channels); Wr32(&h, (uint32_t)sample_rate_hz);
  Wr32(&h, (uint32_t)(sample_rate_hz * num_channels * 2)); Wr16(&h, (uint16_t)(num_channels * 2)); Wr16(&h, 16);
  h.insert(h.end(), {'d', 'a', 't', 'a'}); Wr32(&h, data_bytes);
  std::ofstream out(path.string(), std::ios::binary | std::ios::trunc);
  if (!out.is_open()) { LOG(ERROR) << "Could not open output file " << path.string(); return false; }
  out.write(reinterpret_cast<const char*>(h.data()), h.size());
  out.write(reinterpret_cast<const char*>(samples.data()), data_bytes);
  return out.good();
}

bool EncodeWavs(const std::vector<std::vector<int16_t>>& wav_data, int num_channels, int sample_rate_hz, int bitrate,
                bool enable_preprocessing, bool enable_dtx, const ghc::filesystem::path& model_path,
                std::vector<std::vector<uint8_t>>* encoded_features, int device,
                std::vector<std::vector<int32_t>>* packet_sizes) {
  if (!CheckScope(num_channels, sample_rate_hz, enable_preprocessing, enable_dtx)) return false;
  const int num_bits = BatchBitrateToNumQuantizedBits(bitrate);
  if (num_bits < 0) { LOG(ERROR) << "Bitrate " << bitrate << " bps is not supported by codec."; return false; }
  const int n = (int)wav_data.size();
  encoded_features->assign(n, {});
  if (packet_sizes) packet_sizes->assign(n, {});
  if (n == 0) return true;
  Ctx ctx;
  if (!ctx.Create(model_path, device, n, "encoder")) return false;
  // a DTX LyraEncoder hands its NoiseEstimator the files' rate (lyra_encoder.cc:82-85)
  if (enable_dtx && lyra_hip_set_encoder_sample_rate(ctx.c, sample_rate_hz) != 0) {
    LOG(ERROR) << "Could not set up the noise estimator: " << lyra_hip_last_error(ctx.c);
    return false;
  }
  const int packet_size = BatchBitrateToPacketSize(bitrate);
  const size_t hop_samples = (size_t)sample_rate_hz / 50;   // a 20 ms hop at the files' rate
  const bool resample = sample_rate_hz != kBatchInternalSampleRateHz;
  size_t max_hops = 0;
  for (const auto& w : wav_data) max_hops = std::max(max_hops, w.size() / hop_samples);
  std::vector<int32_t> ids;
  std::vector<int16_t> pcm, pcm16;
  std::vector<uint8_t> packets;
  std::vector<int32_t> sizes;
  for (size_t hop = 0; hop < max_hops; ++hop) {  // streams with a full hop left (encoder_main_lib.cc:71-73)
    ids.clear();
    pcm.clear();
    for (int i = 0; i < n; ++i)
      if ((hop + 1) * hop_samples <= wav_data[i].size()) {
        ids.push_back(i);
        pcm.insert(pcm.end(), wav_data[i].begin() + hop * hop_samples, wav_data[i].begin() + (hop + 1) * hop_samples);
      }
    packets.resize(ids.size() * packet_size);
    const int16_t* hop16 = pcm.data();
    if (resample) {   // the stream's own encoder-side resampler (lyra_encoder.cc:119-122)
      pcm16.resize(ids.size() * kBatchHopSamples);
      if (lyra_hip_resample(ctx.c, LYRA_HIP_SIDE_ENCODER, ids.data(), (int)ids.size(), pcm.data(), (int)hop_samples, sample_rate_hz,
                            kBatchInternalSampleRateHz, pcm16.data()) != 0) {
        LOG(ERROR) << "Unable to resample the hop at sample " << hop * hop_samples << ": " << lyra_hip_last_error(ctx.c);
        return false;
      }
      hop16 = pcm16.data();
    }
    sizes.assign(ids.size(), packet_size);
    if ((enable_dtx ? lyra_hip_encode_dtx(ctx.c, ids.data(), (int)ids.size(), hop16, num_bits, packets.data(), sizes.data())
                    : lyra_hip_encode(ctx.c, ids.data(), (int)ids.size(), hop16, num_bits, packets.data())) != 0) {
      LOG(ERROR) << "Unable to encode features starting at samples at byte " << hop * hop_samples << ": "
                 << lyra_hip_last_error(ctx.c);
      return false;
    }
    for (size_t k = 0; k < ids.size(); ++k) {   // the empty packet of a noise hop appends nothing (encoder_main_lib.cc:77-88)
      auto& dst = (*encoded_features)[ids[k]];
      dst.insert(dst.end(), packets.begin() + k * packet_size, packets.begin() + k * packet_size + sizes[k]);
      if (packet_sizes) (*packet_sizes)[ids[k]].push_back(sizes[k]);
    }
  }
  return true;
}

namespace {
bool EncodeFilesImpl(const std::vector<ghc::filesystem::path>& wav_paths,
                     const std::vector<ghc::filesystem::path>& output_paths, int bitrate, bool enable_preprocessing,
                     bool enable_dtx, const ghc::filesystem::path& model_path, int num_lanes, int device);
bool DecodeFilesImpl(const std::vector<ghc::filesystem::path>& encoded_paths,
                     const std::vector<ghc::filesystem::path>& output_paths, int sample_rate_hz, int bitrate,
                     const ghc::filesystem::path& model_path, int num_lanes, int device);
}  // namespace

bool EncodeFiles(const std::vector<ghc::filesystem::path>& wav_paths,
                 const std::vector<ghc::filesystem::path>& output_paths, int bitrate, bool enable_preprocessing,
                 bool enable_dtx, const ghc::filesystem::path& model_path, int device) {
  return EncodeFilesImpl(wav_paths, output_paths, bitrate, enable_preprocessing, enable_dtx, model_path, -1, device);
}
bool EncodeFilesTimeParallel(const std::vector<ghc::filesystem::path>& wav_paths,
                             const std::vector<ghc::filesystem::path>& output_paths, int bitrate, bool enable_preprocessing,
                             bool enable_dtx, const ghc::filesystem::path& model_path, int num_lanes, int device) {
  return EncodeFilesImpl(wav_paths, output_paths, bitrate, enable_preprocessing, enable_dtx, model_path, std::max(num_lanes, 0),
                         device);
}
bool DecodeFiles(const std::vector<ghc::filesystem::path>& encoded_paths,
                 const std::vector<ghc::filesystem::path>& output_paths, int sample_rate_hz, int bitrate,
                 const ghc::filesystem::path& model_path, int device) {
  return DecodeFilesImpl(encoded_paths, output_paths, sample_rate_hz, bitrate, model_path, -1, device);
}
bool DecodeFilesTimeParallel(const std::vector<ghc::filesystem::path>& encoded_paths,
                             const std::vector<ghc::filesystem::path>& output_paths, int sample_rate_hz, int bitrate,
                             const ghc::filesystem::path& model_path, int num_lanes, int device) {
  return DecodeFilesImpl(encoded_paths, output_paths, sample_rate_hz, bitrate, model_path, std::max(num_lanes, 0), device);
}

namespace {
// num_lanes < 0: hop by hop (EncodeWavs); else time-parallel with that many lanes
bool EncodeFilesImpl(const std::vector<ghc::filesystem::path>& wav_paths,
                     const std::vector<ghc::filesystem::path>& output_paths, int bitrate, bool enable_preprocessing,
                     bool enable_dtx, const ghc::filesystem::path& model_path, int num_lanes, int device) {
  if (wav_paths.size() != output_paths.size()) { LOG(ERROR) << "One output path per input file is required."; return false; }
  std::vector<std::vector<int16_t>> wavs(wav_paths.size());
  int channels = 1, rate = kBatchInternalSampleRateHz;
  for (size_t i = 0; i < wav_paths.size(); ++i) {
    int ch = 0, sr = 0;
    if (!ReadWav16(wav_paths[i], &wavs[i], &ch, &sr)) return false;
    if (i == 0) { channels = ch; rate = sr; }
    if (ch != channels || sr != rate) { LOG(ERROR) << "All files of a batch must share channels / sample rate."; return false; }
  }
  std::vector<std::vector<uint8_t>> encoded;
  if (!(num_lanes < 0 ? EncodeWavs(wavs, channels, rate, bitrate, enable_preprocessing, enable_dtx, model_path, &encoded, device)
                      : EncodeWavsTimeParallel(wavs, channels, rate, bitrate, enable_preprocessing, enable_dtx, model_path,
                                               &encoded, num_lanes, device))) {
    LOG(ERROR) << "Unable to encode features for the batch starting with " << (wav_paths.empty() ? "" : wav_paths[0].string());
    return false;
  }
  for (size_t i = 0; i < output_paths.size(); ++i) {
    std::ofstream out(output_paths[i].string(), std::ios_base::binary | std::ios_base::trunc);
    if (!out.is_open()) { LOG(ERROR) << "Could not open output file " << output_paths[i].string(); return false; }
    out.write(reinterpret_cast<const char*>(encoded[i].data()), encoded[i].size());
  }
  return true;
}
}  // namespace

bool DecodeFeaturesBatch(const std::vector<std::vector<uint8_t>>& packet_streams, int packet_size,
                         const ghc::filesystem::path& model_path, std::vector<std::vector<int16_t>>* decoded_audio,
                         int device) {
  return DecodeFeaturesBatch(packet_streams, packet_size, kBatchInternalSampleRateHz, model_path, decoded_audio, device);
}

bool DecodeFeaturesBatch(const std::vector<std::vector<uint8_t>>& packet_streams, int packet_size, int sample_rate_hz,
                         const ghc::filesystem::path& model_path, std::vector<std::vector<int16_t>>* decoded_audio,
                         int device) {
  if (!CheckScope(1, sample_rate_hz, false, false)) return false;
  const int num_bits = NumBitsOfPacketSize(packet_size);
  if (num_bits < 0) return false;
  const int n = (int)packet_streams.size();
  decoded_audio->assign(n, {});
  if (n == 0) return true;
  if (!WholePackets(packet_streams, packet_size)) return false;
  size_t max_packets = 0;
  for (const auto& p : packet_streams) max_packets = std::max(max_packets, p.size() / packet_size);
  Ctx ctx;
  if (!ctx.Create(model_path, device, n, "decoder")) return false;
  const size_t hop_samples = (size_t)sample_rate_hz / 50;
  const bool resample = sample_rate_hz != kBatchInternalSampleRateHz;
  std::vector<int32_t> ids;
  std::vector<uint8_t> packets;
  std::vector<int16_t> pcm, pcm_ext;
  for (size_t f = 0; f < max_packets; ++f) {
    ids.clear();
    packets.clear();
    for (int i = 0; i < n; ++i)
      if ((f + 1) * packet_size <= packet_streams[i].size()) {
        ids.push_back(i);
        packets.insert(packets.end(), packet_streams[i].begin() + f * packet_size,
                       packet_streams[i].begin() + (f + 1) * packet_size);
      }
    pcm.resize(ids.size() * kBatchHopSamples);
    if (lyra_hip_decode(ctx.c, ids.data(), (int)ids.size(), packets.data(), num_bits, pcm.data()) != 0) {
      LOG(ERROR) << "Could not decode samples: " << lyra_hip_last_error(ctx.c);
      return false;
    }
    if (resample) {   // the stream's own decoder-side resampler (lyra_decoder.cc:107-113)
      pcm_ext.resize(ids.size() * hop_samples);
      if (lyra_hip_resample(ctx.c, LYRA_HIP_SIDE_DECODER, ids.data(), (int)ids.size(), pcm.data(), kBatchHopSamples,
                            kBatchInternalSampleRateHz, sample_rate_hz, pcm_ext.data()) != 0) {
        LOG(ERROR) << "Could not resample the decoded samples: " << lyra_hip_last_error(ctx.c);
        return false;
      }
    }
    const std::vector<int16_t>& hop = resample ? pcm_ext : pcm;
    for (size_t k = 0; k < ids.size(); ++k) {
      auto& dst = (*decoded_audio)[ids[k]];
      dst.insert(dst.end(), hop.begin() + k * hop_samples, hop.begin() + (k + 1) * hop_samples);
    }
  }
  return true;
}

namespace {

// Concatenation of the streams' whole rows (row_sizes[i] units each for stream i) + one span per stream; the lanes are the
// ids behind the files'.  Lanes are capped so that a lane chunk is at least as long as its warm-up (work inflation <= 2).
struct SpanJob {
  std::vector<lyra_hip_span> spans;
  std::vector<int32_t> lanes;
  int64_t frames = 0;
};
template <class T>
SpanJob MakeSpanJob(const std::vector<std::vector<T>>& streams, const std::vector<size_t>& row_sizes, int side, int num_lanes,
                    std::vector<T>* rows) {
  SpanJob job;
  for (size_t i = 0; i < streams.size(); ++i) {
    const int64_t n = (int64_t)(streams[i].size() / row_sizes[i]);
    job.spans.push_back({(int32_t)i, job.frames, n});
    rows->insert(rows->end(), streams[i].begin(), streams[i].begin() + n * row_sizes[i]);
    job.frames += n;
  }
  const int64_t worth = job.frames / (2 * lyra_hip_span_warmup_frames(side));
  const int n_lanes = (int)std::max<int64_t>(0, std::min<int64_t>(num_lanes, worth));
  for (int l = 0; l < n_lanes; ++l) job.lanes.push_back((int32_t)streams.size() + l);
  return job;
}
template <class T>
SpanJob MakeSpanJob(const std::vector<std::vector<T>>& streams, size_t row_size, int side, int num_lanes, std::vector<T>* rows) {
  return MakeSpanJob(streams, std::vector<size_t>(streams.size(), row_size), side, num_lanes, rows);
}
bool HaveSpanCalls(int sample_rate_hz) {
  if (!(lyra_hip_encode_spans && lyra_hip_decode_spans && lyra_hip_span_warmup_frames)) {
    LOG(ERROR) << "This build of the lyra_hip library has no time-parallel span calls.";
    return false;
  }
  if (sample_rate_hz != kBatchInternalSampleRateHz && !(lyra_hip_encode_spans_ext && lyra_hip_decode_spans_ext)) {
    LOG(ERROR) << "This build of the lyra_hip library has no time-parallel span calls at " << sample_rate_hz << " Hz.";
    return false;
  }
  return true;
}
// The span call of a side at a rate.  16 kHz stays on the plain call: it also runs against a library that has no `_ext` calls yet.
int EncodeSpansAt(int rate, lyra_hip_ctx* c, const SpanJob& j, const int16_t* pcm, int num_bits, uint8_t* packets) {
  const int n = (int)j.spans.size(), n_lanes = (int)j.lanes.size();
  if (rate == kBatchInternalSampleRateHz) return lyra_hip_encode_spans(c, j.spans.data(), n, j.lanes.data(), n_lanes, pcm, num_bits, packets);
  return lyra_hip_encode_spans_ext(c, j.spans.data(), n, j.lanes.data(), n_lanes, pcm, rate, num_bits, packets);
}
int DecodeSpansAt(int rate, lyra_hip_ctx* c, const SpanJob& j, const uint8_t* packets, int num_bits, int16_t* pcm) {
  const int n = (int)j.spans.size(), n_lanes = (int)j.lanes.size();
  if (rate == kBatchInternalSampleRateHz) return lyra_hip_decode_spans(c, j.spans.data(), n, j.lanes.data(), n_lanes, packets, num_bits, pcm);
  return lyra_hip_decode_spans_ext(c, j.spans.data(), n, j.lanes.data(), n_lanes, packets, num_bits, rate, pcm);
}
bool HaveSpanDtxCall() {
  if (lyra_hip_encode_spans_dtx) return true;
  LOG(ERROR) << "This build of the lyra_hip library has no time-parallel span call with DTX.";
  return false;
}

// bitrates == nullptr: every hop at `bitrate`; else (*bitrates)[i][h] for hop h of file i, through lyra_hip_encode_spans_mixed
bool EncodeSpans(const std::vector<std::vector<int16_t>>& wav_data, int num_channels, int sample_rate_hz, int bitrate,
                 const std::vector<std::vector<int>>* bitrates, bool enable_preprocessing, bool enable_dtx,
                 const ghc::filesystem::path& model_path, std::vector<std::vector<uint8_t>>* encoded_features, int num_lanes,
                 int device, std::vector<std::vector<int32_t>>* packet_sizes) {
  if (!CheckScope(num_channels, sample_rate_hz, enable_preprocessing, enable_dtx) || !HaveSpanCalls(sample_rate_hz)) return false;
  if (enable_dtx && !HaveSpanDtxCall()) return false;
  if (bitrates && !lyra_hip_encode_spans_mixed) {
    LOG(ERROR) << "This build of the lyra_hip library has no time-parallel span call with per-hop bitrates.";
    return false;
  }
  const int num_bits = bitrates ? 0 : BatchBitrateToNumQuantizedBits(bitrate);
  if (num_bits < 0) { LOG(ERROR) << "Bitrate " << bitrate << " bps is not supported by codec."; return false; }
  const int n = (int)wav_data.size();
  if (bitrates && (int)bitrates->size() != n) { LOG(ERROR) << "One bitrate schedule per file is required."; return false; }
  encoded_features->assign(n, {});
  if (packet_sizes) packet_sizes->assign(n, {});
  if (n == 0) return true;
  std::vector<int16_t> pcm;
  const SpanJob job = MakeSpanJob(wav_data, (size_t)sample_rate_hz / 50, LYRA_HIP_SIDE_ENCODER, num_lanes, &pcm);
  Ctx ctx;
  if (!ctx.Create(model_path, device, n + (int)job.lanes.size(), "encoder")) return false;
  const size_t packet_size = bitrates ? (size_t)LYRA_HIP_MAX_PACKET_BYTES : (size_t)BatchBitrateToPacketSize(bitrate);
  std::vector<uint8_t> packets((size_t)job.frames * packet_size);
  // bytes of every frame's packet: without DTX the packet size, with it or with per-hop bitrates what the call reports
  std::vector<int32_t> sizes((size_t)job.frames, enable_dtx || bitrates ? 0 : (int32_t)packet_size);
  std::vector<int32_t> bits;   // per frame
  for (int i = 0; bitrates && i < n; ++i) {
    if ((int64_t)(*bitrates)[i].size() < job.spans[i].n_frames) { LOG(ERROR) << "A bitrate schedule is shorter than its file."; return false; }
    for (int64_t h = 0; h < job.spans[i].n_frames; ++h) {
      bits.push_back(BatchBitrateToNumQuantizedBits((*bitrates)[i][h]));
      if (bits.back() < 0) { LOG(ERROR) << "Bitrate " << (*bitrates)[i][h] << " bps is not supported by codec."; return false; }
    }
  }
  const int n_lanes = (int)job.lanes.size();
  const bool ok = (!enable_dtx || lyra_hip_set_encoder_sample_rate(ctx.c, sample_rate_hz) == 0) &&
                  (bitrates     ? lyra_hip_encode_spans_mixed(ctx.c, job.spans.data(), n, job.lanes.data(), n_lanes, pcm.data(),
                                                              sample_rate_hz, bits.data(), enable_dtx, packets.data(), sizes.data())
                   : enable_dtx ? lyra_hip_encode_spans_dtx(ctx.c, job.spans.data(), n, job.lanes.data(), n_lanes, pcm.data(),
                                                            sample_rate_hz, num_bits, packets.data(), sizes.data())
                                : EncodeSpansAt(sample_rate_hz, ctx.c, job, pcm.data(), num_bits, packets.data())) == 0;
  if (!ok) {
    LOG(ERROR) << "Unable to encode features: " << lyra_hip_last_error(ctx.c);
    return false;
  }
  for (int i = 0; i < n; ++i) {   // the non-empty packets of every file, in order (encoder_main_lib.cc:77-88)
    auto& dst = (*encoded_features)[i];
    for (int64_t f = job.spans[i].first_frame; f < job.spans[i].first_frame + job.spans[i].n_frames; ++f) {
      dst.insert(dst.end(), packets.begin() + f * packet_size, packets.begin() + f * packet_size + sizes[f]);
      if (packet_sizes) (*packet_sizes)[i].push_back(sizes[f]);
    }
  }
  return true;
}
}  // namespace

bool EncodeWavsTimeParallel(const std::vector<std::vector<int16_t>>& wav_data, int num_channels, int sample_rate_hz,
                            int bitrate, bool enable_preprocessing, bool enable_dtx,
                            const ghc::filesystem::path& model_path, std::vector<std::vector<uint8_t>>* encoded_features,
                            int num_lanes, int device, std::vector<std::vector<int32_t>>* packet_sizes) {
  return EncodeSpans(wav_data, num_channels, sample_rate_hz, bitrate, nullptr, enable_preprocessing, enable_dtx, model_path,
                     encoded_features, num_lanes, device, packet_sizes);
}

bool EncodeWavsTimeParallel(const std::vector<std::vector<int16_t>>& wav_data, int num_channels, int sample_rate_hz,
                            const std::vector<std::vector<int>>& bitrates, bool enable_preprocessing, bool enable_dtx,
                            const ghc::filesystem::path& model_path, std::vector<std::vector<uint8_t>>* encoded_features,
                            std::vector<std::vector<int32_t>>* packet_sizes, int num_lanes, int device) {
  if (!packet_sizes) { LOG(ERROR) << "With per-hop bitrates the packet sizes are part of the result."; return false; }
  return EncodeSpans(wav_data, num_channels, sample_rate_hz, 0, &bitrates, enable_preprocessing, enable_dtx, model_path,
                     encoded_features, num_lanes, device, packet_sizes);
}

bool DecodeFeaturesTimeParallel(const std::vector<std::vector<uint8_t>>& packet_streams, int packet_size,
                                const ghc::filesystem::path& model_path, std::vector<std::vector<int16_t>>* decoded_audio,
                                int num_lanes, int device) {
  return DecodeFeaturesTimeParallel(packet_streams, packet_size, kBatchInternalSampleRateHz, model_path, decoded_audio, num_lanes,
                                    device);
}

bool DecodeFeaturesTimeParallel(const std::vector<std::vector<uint8_t>>& packet_streams, int packet_size, int sample_rate_hz,
                                const ghc::filesystem::path& model_path, std::vector<std::vector<int16_t>>* decoded_audio,
                                int num_lanes, int device) {
  if (!CheckScope(1, sample_rate_hz, false, false)) return false;
  const int num_bits = NumBitsOfPacketSize(packet_size);
  if (num_bits < 0 || !HaveSpanCalls(sample_rate_hz)) return false;
  const int n = (int)packet_streams.size();
  decoded_audio->assign(n, {});
  if (n == 0) return true;
  if (!WholePackets(packet_streams, packet_size)) return false;
  std::vector<uint8_t> packets;
  const SpanJob job = MakeSpanJob(packet_streams, (size_t)packet_size, LYRA_HIP_SIDE_DECODER, num_lanes, &packets);
  Ctx ctx;
  if (!ctx.Create(model_path, device, n + (int)job.lanes.size(), "decoder")) return false;
  const size_t hop_samples = (size_t)sample_rate_hz / 50;
  std::vector<int16_t> pcm((size_t)job.frames * hop_samples);
  if (DecodeSpansAt(sample_rate_hz, ctx.c, job, packets.data(), num_bits, pcm.data()) != 0) {
    LOG(ERROR) << "Could not decode samples: " << lyra_hip_last_error(ctx.c);
    return false;
  }
  for (int i = 0; i < n; ++i)
    (*decoded_audio)[i].assign(pcm.begin() + job.spans[i].first_frame * hop_samples,
                               pcm.begin() + (job.spans[i].first_frame + job.spans[i].n_frames) * hop_samples);
  return true;
}

namespace {
// packet_sizes[i][h] is 0 or packet_size (packet_size 0: or any size of the codec) and the non-empty packets of stream i are
// exactly packet_streams[i]
bool SizesMatch(const std::vector<std::vector<uint8_t>>& packet_streams, const std::vector<std::vector<int32_t>>& packet_sizes,
                int packet_size) {
  if (packet_sizes.size() != packet_streams.size()) { LOG(ERROR) << "One list of packet sizes per stream is required."; return false; }
  for (size_t i = 0; i < packet_streams.size(); ++i) {
    size_t bytes = 0;
    for (int32_t b : packet_sizes[i]) {
      if (b != 0 && (packet_size ? b != packet_size : b != 8 && b != 15 && b != LYRA_HIP_MAX_PACKET_BYTES)) {
        LOG(ERROR) << "A packet size (" << b << ") is neither 0 nor " << (packet_size ? std::to_string(packet_size) : "8, 15 or 23") << ".";
        return false;
      }
      bytes += (size_t)b;
    }
    if (bytes != packet_streams[i].size()) { LOG(ERROR) << "The packet sizes do not add up to the encoded stream."; return false; }
  }
  return true;
}
}  // namespace

bool DecodeFeaturesBatch(const std::vector<std::vector<uint8_t>>& packet_streams,
                         const std::vector<std::vector<int32_t>>& packet_sizes, int packet_size, int sample_rate_hz,
                         const ghc::filesystem::path& model_path, std::vector<std::vector<int16_t>>* decoded_audio, int device) {
  if (!CheckScope(1, sample_rate_hz, false, false) || NumBitsOfPacketSize(packet_size) < 0) return false;
  if (!SizesMatch(packet_streams, packet_sizes, packet_size)) return false;
  const int n = (int)packet_streams.size();
  decoded_audio->assign(n, {});
  if (n == 0) return true;
  auto decoder = BatchLyraDecoder::Create(sample_rate_hz, 1, model_path, n, device);
  if (!decoder) return false;
  size_t hops = 0;
  for (const auto& v : packet_sizes) hops = std::max(hops, v.size());
  const size_t hop_samples = (size_t)sample_rate_hz / 50;
  std::vector<size_t> at((size_t)n, 0);   // bytes of stream i consumed
  std::vector<int32_t> ids;
  std::vector<uint8_t> packets;
  std::vector<int16_t> pcm((size_t)n * hop_samples);
  for (size_t h = 0; h < hops; ++h) {
    ids.clear();
    packets.clear();
    for (int i = 0; i < n; ++i)
      if (h < packet_sizes[i].size() && packet_sizes[i][h]) {
        ids.push_back(i);
        packets.insert(packets.end(), packet_streams[i].begin() + at[i], packet_streams[i].begin() + at[i] + packet_size);
        at[i] += (size_t)packet_size;
      }
    if (!ids.empty() && !decoder->SetEncodedPackets(absl::MakeConstSpan(ids), absl::MakeConstSpan(packets))) return false;
    if (!decoder->DecodeSamples((int)hop_samples, absl::Span<int16_t>(pcm.data(), pcm.size()))) return false;
    for (int i = 0; i < n; ++i)   // a stream that has ended goes on concealing; its hops are dropped
      if (h < packet_sizes[i].size())
        (*decoded_audio)[i].insert((*decoded_audio)[i].end(), pcm.begin() + i * hop_samples, pcm.begin() + (i + 1) * hop_samples);
  }
  return true;
}

namespace {
// packet_size 0: every hop's size is its own (8 / 15 / 23), through lyra_hip_decode_spans_lossy_mixed
bool DecodeSpansLossy(const std::vector<std::vector<uint8_t>>& packet_streams,
                      const std::vector<std::vector<int32_t>>& packet_sizes, int packet_size, int sample_rate_hz,
                      const ghc::filesystem::path& model_path, std::vector<std::vector<int16_t>>* decoded_audio, int num_lanes,
                      int device) {
  if (!CheckScope(1, sample_rate_hz, false, false)) return false;
  const int num_bits = packet_size ? NumBitsOfPacketSize(packet_size) : 0;
  if (num_bits < 0 || !HaveSpanCalls(sample_rate_hz)) return false;
  if (packet_size ? !lyra_hip_decode_spans_lossy : !lyra_hip_decode_spans_lossy_mixed) {
    LOG(ERROR) << "This build of the lyra_hip library has no time-parallel span call for missing packets"
               << (packet_size ? "." : " of per-hop sizes.");
    return false;
  }
  const int row_size = packet_size ? packet_size : LYRA_HIP_MAX_PACKET_BYTES;
  if (!SizesMatch(packet_streams, packet_sizes, packet_size)) return false;
  const int n = (int)packet_streams.size();
  decoded_audio->assign(n, {});
  if (n == 0) return true;
  // frame-major: one packet row per hop (zeros where there is none) and its size
  SpanJob job;
  std::vector<uint8_t> packets;
  std::vector<int32_t> sizes;
  for (int i = 0; i < n; ++i) {
    job.spans.push_back({(int32_t)i, job.frames, (int64_t)packet_sizes[i].size()});
    size_t at = 0;
    for (int32_t b : packet_sizes[i]) {
      packets.insert(packets.end(), (size_t)row_size, 0);
      if (b) std::copy(packet_streams[i].begin() + at, packet_streams[i].begin() + at + b, packets.end() - row_size);
      at += (size_t)b;
      sizes.push_back(b);
    }
    job.frames += (int64_t)packet_sizes[i].size();
  }
  const int64_t worth = job.frames / (2 * lyra_hip_span_warmup_frames(LYRA_HIP_SIDE_DECODER));
  for (int l = 0; l < (int)std::max<int64_t>(0, std::min<int64_t>(num_lanes, worth)); ++l) job.lanes.push_back(n + l);
  Ctx ctx;
  if (!ctx.Create(model_path, device, n + (int)job.lanes.size(), "decoder")) return false;
  const size_t hop_samples = (size_t)sample_rate_hz / 50;
  const bool ext = sample_rate_hz != kBatchInternalSampleRateHz;
  std::vector<int16_t> pcm16((size_t)job.frames * kBatchHopSamples), pcm_ext(ext ? (size_t)job.frames * hop_samples : 0);
  const int n_lanes = (int)job.lanes.size();
  int16_t* const ext_out = ext ? pcm_ext.data() : nullptr;
  if ((packet_size ? lyra_hip_decode_spans_lossy(ctx.c, job.spans.data(), n, job.lanes.data(), n_lanes, packets.data(), sizes.data(),
                                                 num_bits, sample_rate_hz, pcm16.data(), ext_out, nullptr, nullptr)
                   : lyra_hip_decode_spans_lossy_mixed(ctx.c, job.spans.data(), n, job.lanes.data(), n_lanes, packets.data(),
                                                       sizes.data(), sample_rate_hz, pcm16.data(), ext_out, nullptr, nullptr)) != 0) {
    LOG(ERROR) << "Could not decode samples: " << lyra_hip_last_error(ctx.c);
    return false;
  }
  const std::vector<int16_t>& pcm = ext ? pcm_ext : pcm16;
  for (int i = 0; i < n; ++i)
    (*decoded_audio)[i].assign(pcm.begin() + job.spans[i].first_frame * hop_samples,
                               pcm.begin() + (job.spans[i].first_frame + job.spans[i].n_frames) * hop_samples);
  return true;
}
}  // namespace

bool DecodeFeaturesTimeParallel(const std::vector<std::vector<uint8_t>>& packet_streams,
                                const std::vector<std::vector<int32_t>>& packet_sizes, int packet_size, int sample_rate_hz,
                                const ghc::filesystem::path& model_path, std::vector<std::vector<int16_t>>* decoded_audio,
                                int num_lanes, int device) {
  if (NumBitsOfPacketSize(packet_size) < 0) return false;
  return DecodeSpansLossy(packet_streams, packet_sizes, packet_size, sample_rate_hz, model_path, decoded_audio, num_lanes, device);
}

bool DecodeFeaturesTimeParallel(const std::vector<std::vector<uint8_t>>& packet_streams,
                                const std::vector<std::vector<int32_t>>& packet_sizes, int sample_rate_hz,
                                const ghc::filesystem::path& model_path, std::vector<std::vector<int16_t>>* decoded_audio,
                                int num_lanes, int device) {
  return DecodeSpansLossy(packet_streams, packet_sizes, 0, sample_rate_hz, model_path, decoded_audio, num_lanes, device);
}

// ---- files of any rate side by side (include/lyra_hip_spans_packed.h) -----------------------------------------------------------
namespace {
bool HavePackedSpanCalls() {
  if (lyra_hip_encode_spans_packed && lyra_hip_decode_spans_lossy_packed && lyra_hip_decode_spans_packed &&
      lyra_hip_span_warmup_frames)
    return true;
  LOG(ERROR) << "This build of the lyra_hip library has no packed per-rate span calls.";
  return false;
}
bool CheckRates(const std::vector<int>& sample_rates_hz, size_t n) {
  if (sample_rates_hz.size() != n) { LOG(ERROR) << "One sample rate per file is required."; return false; }
  for (int r : sample_rates_hz)
    if (!CheckScope(1, r, false, false)) return false;
  return true;
}

bool EncodeSpansAnyRate(const std::vector<std::vector<int16_t>>& wav_data, const std::vector<int>& sample_rates_hz, int bitrate,
                        const std::vector<std::vector<int>>* bitrates, bool enable_dtx, const ghc::filesystem::path& model_path,
                        std::vector<std::vector<uint8_t>>* encoded_features, std::vector<std::vector<int32_t>>* packet_sizes,
                        int num_lanes, int device) {
  if (!HavePackedSpanCalls() || !CheckRates(sample_rates_hz, wav_data.size())) return false;
  const int uniform_bits = bitrates ? 0 : BatchBitrateToNumQuantizedBits(bitrate);
  if (uniform_bits < 0) { LOG(ERROR) << "Bitrate " << bitrate << " bps is not supported by codec."; return false; }
  const int n = (int)wav_data.size();
  if (bitrates && (int)bitrates->size() != n) { LOG(ERROR) << "One bitrate schedule per file is required."; return false; }
  encoded_features->assign(n, {});
  if (packet_sizes) packet_sizes->assign(n, {});
  if (n == 0) return true;
  std::vector<size_t> hops((size_t)n);
  for (int i = 0; i < n; ++i) hops[i] = (size_t)sample_rates_hz[i] / 50;
  std::vector<int16_t> pcm;   // the files' whole hops back to back: the packed layout with ext_offsets == NULL
  const SpanJob job = MakeSpanJob(wav_data, hops, LYRA_HIP_SIDE_ENCODER, num_lanes, &pcm);
  std::vector<int32_t> bits, rates(sample_rates_hz.begin(), sample_rates_hz.end());
  for (int i = 0; i < n; ++i) {
    if (bitrates && (int64_t)(*bitrates)[i].size() < job.spans[i].n_frames) { LOG(ERROR) << "A bitrate schedule is shorter than its file."; return false; }
    for (int64_t h = 0; h < job.spans[i].n_frames; ++h) {
      bits.push_back(bitrates ? BatchBitrateToNumQuantizedBits((*bitrates)[i][h]) : uniform_bits);
      if (bits.back() < 0) { LOG(ERROR) << "Bitrate " << (*bitrates)[i][h] << " bps is not supported by codec."; return false; }
    }
  }
  bits.push_back(4);   // (never empty)
  Ctx ctx;
  if (!ctx.Create(model_path, device, n + (int)job.lanes.size(), "encoder")) return false;
  const size_t row = (size_t)LYRA_HIP_MAX_PACKET_BYTES;
  std::vector<uint8_t> packets((size_t)job.frames * row + 1);
  std::vector<int32_t> sizes((size_t)job.frames + 1, 0);
  if (lyra_hip_encode_spans_packed(ctx.c, job.spans.data(), n, job.lanes.data(), (int)job.lanes.size(), pcm.data(),
                                   (long long)pcm.size(), nullptr, rates.data(), bits.data(), enable_dtx, packets.data(),
                                   sizes.data()) != 0) {
    LOG(ERROR) << "Unable to encode features: " << lyra_hip_last_error(ctx.c);
    return false;
  }
  for (int i = 0; i < n; ++i) {   // the non-empty packets of every file, in order (encoder_main_lib.cc:77-88)
    auto& dst = (*encoded_features)[i];
    for (int64_t f = job.spans[i].first_frame; f < job.spans[i].first_frame + job.spans[i].n_frames; ++f) {
      dst.insert(dst.end(), packets.begin() + f * row, packets.begin() + f * row + sizes[f]);
      if (packet_sizes) (*packet_sizes)[i].push_back(sizes[f]);
    }
  }
  return true;
}
}  // namespace

bool EncodeWavsAnyRateTimeParallel(const std::vector<std::vector<int16_t>>& wav_data, const std::vector<int>& sample_rates_hz,
                                   int bitrate, bool enable_dtx, const ghc::filesystem::path& model_path,
                                   std::vector<std::vector<uint8_t>>* encoded_features,
                                   std::vector<std::vector<int32_t>>* packet_sizes, int num_lanes, int device) {
  return EncodeSpansAnyRate(wav_data, sample_rates_hz, bitrate, nullptr, enable_dtx, model_path, encoded_features, packet_sizes,
                            num_lanes, device);
}

bool EncodeWavsAnyRateTimeParallel(const std::vector<std::vector<int16_t>>& wav_data, const std::vector<int>& sample_rates_hz,
                                   const std::vector<std::vector<int>>& bitrates, bool enable_dtx,
                                   const ghc::filesystem::path& model_path, std::vector<std::vector<uint8_t>>* encoded_features,
                                   std::vector<std::vector<int32_t>>* packet_sizes, int num_lanes, int device) {
  if (!packet_sizes) { LOG(ERROR) << "With per-hop bitrates the packet sizes are part of the result."; return false; }
  return EncodeSpansAnyRate(wav_data, sample_rates_hz, 0, &bitrates, enable_dtx, model_path, encoded_features, packet_sizes,
                            num_lanes, device);
}

bool DecodeFeaturesAnyRateTimeParallel(const std::vector<std::vector<uint8_t>>& packet_streams,
                                       const std::vector<std::vector<int32_t>>& packet_sizes,
                                       const std::vector<int>& sample_rates_hz, const ghc::filesystem::path& model_path,
                                       std::vector<std::vector<int16_t>>* decoded_audio, int num_lanes, int device) {
  if (!HavePackedSpanCalls() || !CheckRates(sample_rates_hz, packet_streams.size())) return false;
  if (!SizesMatch(packet_streams, packet_sizes, 0)) return false;
  const int n = (int)packet_streams.size();
  decoded_audio->assign(n, {});
  if (n == 0) return true;
  // every hop with a packet of one size: the call without loss handling, on packet rows of that size
  int one_size = -1;
  for (const auto& v : packet_sizes)
    for (int32_t b : v) one_size = one_size < 0 || one_size == b ? b : 0;
  const bool plain = one_size > 0;
  const size_t row = plain ? (size_t)one_size : (size_t)LYRA_HIP_MAX_PACKET_BYTES;
  SpanJob job;
  std::vector<uint8_t> packets;
  std::vector<int32_t> sizes, rates(sample_rates_hz.begin(), sample_rates_hz.end());
  long long samples = 0;
  std::vector<long long> at_sample((size_t)n);
  for (int i = 0; i < n; ++i) {
    job.spans.push_back({(int32_t)i, job.frames, (int64_t)packet_sizes[i].size()});
    size_t at = 0;
    for (int32_t b : packet_sizes[i]) {
      packets.insert(packets.end(), row, 0);
      if (b) std::copy(packet_streams[i].begin() + at, packet_streams[i].begin() + at + b, packets.end() - row);
      at += (size_t)b;
      sizes.push_back(b);
    }
    job.frames += (int64_t)packet_sizes[i].size();
    at_sample[i] = samples;   // the back-to-back layout (lyra_hip_spans_packed_layout)
    samples += (long long)packet_sizes[i].size() * (sample_rates_hz[i] / 50);
  }
  const int64_t worth = job.frames / (2 * lyra_hip_span_warmup_frames(LYRA_HIP_SIDE_DECODER));
  for (int l = 0; l < (int)std::max<int64_t>(0, std::min<int64_t>(num_lanes, worth)); ++l) job.lanes.push_back(n + l);
  Ctx ctx;
  if (!ctx.Create(model_path, device, n + (int)job.lanes.size(), "decoder")) return false;
  packets.push_back(0);   // (never empty)
  sizes.push_back(0);
  std::vector<int16_t> pcm((size_t)samples + 1);
  const int n_lanes = (int)job.lanes.size();
  if ((plain ? lyra_hip_decode_spans_packed(ctx.c, job.spans.data(), n, job.lanes.data(), n_lanes, packets.data(),
                                            NumBitsOfPacketSize(one_size), rates.data(), nullptr, pcm.data(), samples, nullptr)
             : lyra_hip_decode_spans_lossy_packed(ctx.c, job.spans.data(), n, job.lanes.data(), n_lanes, packets.data(), sizes.data(),
                                                  rates.data(), nullptr, pcm.data(), samples, nullptr, nullptr, nullptr)) != 0) {
    LOG(ERROR) << "Could not decode samples: " << lyra_hip_last_error(ctx.c);
    return false;
  }
  for (int i = 0; i < n; ++i)
    (*decoded_audio)[i].assign(pcm.begin() + at_sample[i],
                               pcm.begin() + at_sample[i] + (long long)packet_sizes[i].size() * (sample_rates_hz[i] / 50));
  return true;
}

bool EncodeFilesAnyRateTimeParallel(const std::vector<ghc::filesystem::path>& wav_paths,
                                    const std::vector<ghc::filesystem::path>& output_paths, int bitrate, bool enable_dtx,
                                    const ghc::filesystem::path& model_path, int num_lanes, int device) {
  if (wav_paths.size() != output_paths.size()) { LOG(ERROR) << "One output path per input file is required."; return false; }
  std::vector<std::vector<int16_t>> wavs(wav_paths.size());
  std::vector<int> rates(wav_paths.size());
  for (size_t i = 0; i < wav_paths.size(); ++i) {
    int ch = 0;
    if (!ReadWav16(wav_paths[i], &wavs[i], &ch, &rates[i]) || !CheckScope(ch, rates[i], false, enable_dtx)) return false;
  }
  std::vector<std::vector<uint8_t>> encoded;
  if (!EncodeWavsAnyRateTimeParallel(wavs, rates, bitrate, enable_dtx, model_path, &encoded, nullptr, std::max(num_lanes, 0), device)) {
    LOG(ERROR) << "Unable to encode features for the batch starting with " << (wav_paths.empty() ? "" : wav_paths[0].string());
    return false;
  }
  for (size_t i = 0; i < output_paths.size(); ++i) {
    std::ofstream out(output_paths[i].string(), std::ios_base::binary | std::ios_base::trunc);
    if (!out.is_open()) { LOG(ERROR) << "Could not open output file " << output_paths[i].string(); return false; }
    out.write(reinterpret_cast<const char*>(encoded[i].data()), encoded[i].size());
  }
  return true;
}

bool DecodeFilesAnyRateTimeParallel(const std::vector<ghc::filesystem::path>& encoded_paths,
                                    const std::vector<ghc::filesystem::path>& output_paths,
                                    const std::vector<int>& sample_rates_hz, int bitrate, const ghc::filesystem::path& model_path,
                                    int num_lanes, int device) {
  if (encoded_paths.size() != output_paths.size()) { LOG(ERROR) << "One output path per input file is required."; return false; }
  if (!CheckRates(sample_rates_hz, encoded_paths.size())) return false;
  if (BatchBitrateToNumQuantizedBits(bitrate) < 0) { LOG(ERROR) << "Bitrate " << bitrate << " bps is not supported by codec."; return false; }
  const int packet_size = BatchBitrateToPacketSize(bitrate);
  std::vector<std::vector<uint8_t>> streams(encoded_paths.size());
  std::vector<std::vector<int32_t>> sizes(encoded_paths.size());
  for (size_t i = 0; i < encoded_paths.size(); ++i) {
    std::ifstream in(encoded_paths[i].string(), std::ios::binary);
    if (!in.is_open()) { LOG(ERROR) << "Could not open " << encoded_paths[i].string(); return false; }
    streams[i].assign((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    sizes[i].assign(streams[i].size() / (size_t)packet_size, packet_size);
  }
  if (!WholePackets(streams, packet_size)) return false;
  std::vector<std::vector<int16_t>> audio;
  if (!DecodeFeaturesAnyRateTimeParallel(streams, sizes, sample_rates_hz, model_path, &audio, std::max(num_lanes, 0), device))
    return false;
  for (size_t i = 0; i < output_paths.size(); ++i)
    if (!WriteWav16(output_paths[i], audio[i], 1, sample_rates_hz[i])) return false;
  return true;
}

namespace {
bool DecodeFilesImpl(const std::vector<ghc::filesystem::path>& encoded_paths,
                     const std::vector<ghc::filesystem::path>& output_paths, int sample_rate_hz, int bitrate,
                     const ghc::filesystem::path& model_path, int num_lanes, int device) {
  if (encoded_paths.size() != output_paths.size()) { LOG(ERROR) << "One output path per input file is required."; return false; }
  if (!CheckScope(1, sample_rate_hz, false, false)) return false;
  if (BatchBitrateToNumQuantizedBits(bitrate) < 0) { LOG(ERROR) << "Bitrate " << bitrate << " bps is not supported by codec."; return false; }
  std::vector<std::vector<uint8_t>> streams(encoded_paths.size());
  for (size_t i = 0; i < encoded_paths.size(); ++i) {
    std::ifstream in(encoded_paths[i].string(), std::ios::binary);
    if (!in.is_open()) { LOG(ERROR) << "Could not open " << encoded_paths[i].string(); return false; }
    streams[i].assign((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  }
  std::vector<std::vector<int16_t>> audio;
  const int packet_size = BatchBitrateToPacketSize(bitrate);
  if (!(num_lanes < 0 ? DecodeFeaturesBatch(streams, packet_size, sample_rate_hz, model_path, &audio, device)
                      : DecodeFeaturesTimeParallel(streams, packet_size, sample_rate_hz, model_path, &audio, num_lanes, device)))
    return false;
  for (size_t i = 0; i < output_paths.size(); ++i)
    if (!WriteWav16(output_paths[i], audio[i], 1, sample_rate_hz)) return false;
  return true;
}
}  // namespace

}  // namespace codec
}  // namespace chromemedia
