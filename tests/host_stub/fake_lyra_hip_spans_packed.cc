// fake_lyra_hip_spans_packed.cc -- TEST INFRASTRUCTURE, linked BESIDE fake_lyra_hip_codec.cc: a CPU stand-in for the three
// host-buffer calls of include/lyra_hip_spans_packed.h, so that the any-rate file functions of lyra_amd/host/lyra_file_codec.cc
// run in the CPU suite.  Each call goes frame by frame through the other fake's own exported functions -- lyra_hip_resample,
// lyra_hip_encode[_dtx], lyra_hip_decode -- with the stream of the span, so a span handled at the wrong rate, from the wrong
// offset or in the wrong order changes the output.  The argument checks are the library's own (spans_packed_plan.h).
// The lossy form serves hops that all carry a packet; a hop without one is refused: the stand-in has no concealment.
// Never linked into the product.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/lyra_hip_spans_packed.h"
#include "../../lyra_amd/csrc/spans_packed_plan.h"

namespace {
bool resolve(const lyra_hip_span* spans, int n_spans, const int32_t* rates, const long long* ext_offsets, long long n_ext,
             std::vector<long long>* base) {
  if (!spans || n_spans <= 0 || !rates) return false;
  base->assign((size_t)n_spans, 0);
  if (ext_offsets) base->assign(ext_offsets, ext_offsets + n_spans);
  else if (lyra::spk::layout(spans, n_spans, rates, base->data()) < 0) return false;
  return lyra::spk::check(spans, n_spans, rates, base->data(), n_ext) == lyra::spk::PK_OK;
}

int decode_frames(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const uint8_t* packets, size_t row,
                  const int32_t* packet_bytes, int num_bits, const int32_t* rates, int16_t* pcm16, int16_t* pcm_ext, long long n_ext,
                  const long long* ext_offsets) {
  std::vector<long long> base;
  if (!resolve(spans, n_spans, rates, ext_offsets, n_ext, &base)) return LYRA_HIP_EINVAL;
  for (int s = 0; s < n_spans; ++s) {
    const int hop = rates[s] / 50;
    for (int64_t k = 0; k < spans[s].n_frames; ++k) {
      const int64_t f = spans[s].first_frame + k;
      if (packet_bytes && packet_bytes[f] != 8 && packet_bytes[f] != 15 && packet_bytes[f] != 23) return LYRA_HIP_EINVAL;
      int16_t hop16[320];
      int rc = lyra_hip_decode(c, &spans[s].stream_id, 1, packets + (size_t)f * row, packet_bytes ? packet_bytes[f] * 8 : num_bits, hop16);
      if (rc) return rc;
      if (pcm16) std::memcpy(pcm16 + f * 320, hop16, sizeof hop16);
      int16_t* out = pcm_ext + base[(size_t)s] + k * hop;
      if (rates[s] == 16000) std::memcpy(out, hop16, sizeof hop16);
      else if ((rc = lyra_hip_resample(c, LYRA_HIP_SIDE_DECODER, &spans[s].stream_id, 1, hop16, 320, 16000, rates[s], out))) return rc;
    }
  }
  return 0;
}
}  // namespace

extern "C" {

int lyra_hip_span_warmup_frames(int side) { return side == LYRA_HIP_SIDE_ENCODER ? 7 : 9; }   // (any positive number: no lanes here)

int lyra_hip_encode_spans_packed(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t*, int,
                                 const int16_t* pcm_ext, long long n_ext_samples, const long long* ext_offsets,
                                 const int32_t* sample_rates, const int32_t* num_bits, int dtx, uint8_t* packets,
                                 int32_t* packet_bytes) {
  std::vector<long long> base;
  if (!num_bits || !packet_bytes || !resolve(spans, n_spans, sample_rates, ext_offsets, n_ext_samples, &base)) return LYRA_HIP_EINVAL;
  for (int s = 0; s < n_spans; ++s) {
    const int hop = sample_rates[s] / 50;
    for (int64_t k = 0; k < spans[s].n_frames; ++k) {
      const int64_t f = spans[s].first_frame + k;
      const int16_t* in = pcm_ext + base[(size_t)s] + k * hop;
      int16_t hop16[320];
      int rc = 0;
      if (sample_rates[s] == 16000) std::memcpy(hop16, in, sizeof hop16);
      else if ((rc = lyra_hip_resample(c, LYRA_HIP_SIDE_ENCODER, &spans[s].stream_id, 1, in, hop, sample_rates[s], 16000, hop16))) return rc;
      uint8_t* row = packets + (size_t)f * LYRA_HIP_MAX_PACKET_BYTES;
      std::memset(row, 0, LYRA_HIP_MAX_PACKET_BYTES);
      packet_bytes[f] = (num_bits[f] + 7) / 8;
      rc = dtx ? lyra_hip_encode_dtx(c, &spans[s].stream_id, 1, hop16, num_bits[f], row, &packet_bytes[f])
               : lyra_hip_encode(c, &spans[s].stream_id, 1, hop16, num_bits[f], row);
      if (rc) return rc;
    }
  }
  return 0;
}

int lyra_hip_decode_spans_lossy_packed(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t*, int,
                                       const uint8_t* packets, const int32_t* packet_bytes, const int32_t* sample_rates,
                                       int16_t* pcm16, int16_t* pcm_ext, long long n_ext_samples, const long long* ext_offsets,
                                       int32_t*, int32_t*) {
  if (!packet_bytes) return LYRA_HIP_EINVAL;
  return decode_frames(c, spans, n_spans, packets, LYRA_HIP_MAX_PACKET_BYTES, packet_bytes, 0, sample_rates, pcm16, pcm_ext,
                       n_ext_samples, ext_offsets);
}

int lyra_hip_decode_spans_packed(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t*, int,
                                 const uint8_t* packets, int num_bits, const int32_t* sample_rates, int16_t* pcm16, int16_t* pcm_ext,
                                 long long n_ext_samples, const long long* ext_offsets) {
  return decode_frames(c, spans, n_spans, packets, (size_t)(num_bits + 7) / 8, nullptr, num_bits, sample_rates, pcm16, pcm_ext,
                       n_ext_samples, ext_offsets);
}

}  // extern "C"
