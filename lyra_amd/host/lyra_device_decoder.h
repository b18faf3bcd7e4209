// lyra_device_decoder.h -- DeviceLyraDecoder: LyraDecoder for many streams with the WHOLE packet-loss state machine on the
// device (include/lyra_hip.h lyra_hip_decode_samples_dev), for receivers whose requests are not tied to the 20 ms hop: an
// audio device that pulls 10 ms while packets arrive every 20 ms, a jitter buffer that hands packets over early or late.
// BatchLyraDecoder's method names and signatures (lyra_batch_codec.h), so one can stand in for the other; the differences:
//   - a request is 0 .. sample_rate_hz / 50 samples and a whole number of 16 kHz samples (any n at 8 and 16 kHz, even n at
//     32 kHz, multiples of 3 at 48 kHz; 10 ms qualifies at every rate).  Other sizes are refused (false / nullopt +
//     LOG(ERROR)): they are AnySizeDeviceLyraDecoder's (lyra_device_decoder_any.h, up to four hops) or BatchLyraDecoder's;
//   - every stream holds at most LYRA_HIP_DECODE_SAMPLES_FIFO packets whose hop has not started; SetEncodedPackets refuses
//     the whole call when one of its streams is full (the reference's queue is unbounded);
//   - per request the host does integer bookkeeping only (decode_samples_plan.h, the function the device runs): one
//     upload of the packets, one device call, one download.
// A second packet for a stream before the next request goes to the device in a call of its own, which is ended at once; it
// cannot overtake requests in flight, so it is refused until WaitDecoded has delivered every DecodeSamplesAsync request.
#ifndef LYRA_AMD_HOST_LYRA_DEVICE_DECODER_H_
#define LYRA_AMD_HOST_LYRA_DEVICE_DECODER_H_

#include <cstdint>
#include <memory>
#include <optional>
#include <vector>

#include "../csrc/decode_samples_plan.h"
#include "lyra_batch_codec.h"

namespace chromemedia {
namespace codec {

class DeviceLyraDecoder {
 public:
  // Arguments of LyraDecoder::Create (lyra_decoder.h:54-56) + the number of streams.
  static std::unique_ptr<DeviceLyraDecoder> Create(int sample_rate_hz, int num_channels,
                                                   const ghc::filesystem::path& model_path, int num_streams,
                                                   int device = 0);
  ~DeviceLyraDecoder();
  bool SetEncodedPackets(absl::Span<const uint8_t> encoded);
  bool SetEncodedPackets(absl::Span<const int32_t> streams, absl::Span<const uint8_t> encoded);
  std::optional<std::vector<int16_t>> DecodeSamples(int num_samples);
  bool DecodeSamples(int num_samples, absl::Span<int16_t> out);
  bool DecodeSamplesAsync(int num_samples);
  bool WaitDecoded(absl::Span<int16_t> out);
  int requests_in_flight() const { return static_cast<int>(pending_.size()); }
  int sample_rate_hz() const { return sample_rate_hz_; }
  int num_channels() const { return 1; }
  int frame_rate() const { return kBatchFrameRate; }
  bool is_comfort_noise(int stream) const;
  int num_streams() const { return num_streams_; }
  // One stream's DECODER state -- networks, estimator, resampler, comfort noise, the loss state machine with its waiting
  // packets and hops in progress -- as a blob for ImportStream of any DeviceLyraDecoder of the same sample rate, under any
  // stream index (BatchLyraEncoder::ExportStream's format, kind "device decoder").  A packet staged for the stream is handed
  // to the device first, so it is part of the blob.  ImportStream rebuilds the stream's host mirror from the blob and drops a
  // packet staged for the target.  Both refuse while requests are in flight.  (defined in lyra_stream_state.cc)
  std::optional<std::vector<uint8_t>> ExportStream(int stream);
  bool ImportStream(int stream, absl::Span<const uint8_t> blob);

 private:
  DeviceLyraDecoder(lyra_hip_ctx* ctx, int sample_rate_hz, int num_streams);
  bool Begin(int num_samples);   // the staged packets + a request of num_samples to the device, host mirror advanced
  bool FlushStaged();            // the staged packets alone: a device call of 0 samples, ended at once
  bool StreamIdle(const char* method, int stream) const;   // (lyra_stream_state.cc)

  lyra_hip_ctx* ctx_;
  int sample_rate_hz_;
  int num_streams_;
  bool failed_ = false;                        // a device call failed: every further call is refused
  std::vector<int32_t> all_ids_;               // 0 .. num_streams - 1
  std::vector<lyra::DsState> state_;           // the device's per-stream integers, mirrored (never read back)
  std::vector<uint8_t> staged_;                // [num_streams][LYRA_HIP_MAX_PACKET_BYTES] packets for the next device call
  std::vector<int32_t> staged_bytes_;          // [num_streams] 0 = none
  std::vector<int> pending_;                   // num_samples of the requests begun, oldest first (device calls of 0 samples
                                               // made for a second packet are ended at once and never listed)
};

}  // namespace codec
}  // namespace chromemedia
#endif
