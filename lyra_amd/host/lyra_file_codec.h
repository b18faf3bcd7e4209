// lyra_file_codec.h -- whole-file transcodes, many files at once: batched twins of the CLI
// library functions EncodeWav / EncodeFile (cli_example/encoder_main_lib.h:29-38, .cc:42-133) and DecodeFeatures /
// DecodeFile (cli_example/decoder_main_lib.h:51-69).  File i is stream i of one GPU context; files of different
// lengths simply leave the batch when they run out of full 20 ms hops (the C ABI takes any subset of stream ids
// per call).  The ...TimeParallel forms below give the same bytes for long files at batch throughput.  The `.lyra` format is the reference's: the packets of a stream concatenated, nothing else
// (encoder_main_lib.cc:120-130; a trailing partial hop is dropped, :71-73).
//
// Scope: mono 16-bit WAV at 8, 16, 32 or 48 kHz like the reference's EncodeFile / DecodeFile (the files of one batch share
// their rate); at a rate other than 16 kHz every stream runs through its own resampler on the device, lyra_hip_resample per
// hop or, in the time-parallel forms, one pass inside lyra_hip_encode_spans_ext / lyra_hip_decode_spans_ext.  A hop is
// sample_rate_hz / 50 samples.  enable_dtx is encoder_main's --enable_dtx (lyra_hip_set_encoder_sample_rate(rate), then
// lyra_hip_resample + lyra_hip_encode_dtx per hop or, time-parallel, lyra_hip_encode_spans_dtx): a noise hop's empty packet
// appends nothing, so the output is the concatenation of the non-empty packets (encoder_main_lib.cc:77-88) and, like the
// reference's, cannot be cut into hops again without the sizes -- packet_sizes returns them.  The file functions do not decode
// such a file; the DecodeFeatures forms that take packet_sizes do decode such a stream, and one captured from a lossy link
// (a loss trace has the same shape: 0 = no packet this hop): concealment, comfort noise and cross-fades as LyraDecoder's.
// No preprocessing / packet-loss simulation: those are refused.
#ifndef LYRA_AMD_HOST_LYRA_FILE_CODEC_H_
#define LYRA_AMD_HOST_LYRA_FILE_CODEC_H_
#include <cstdint>
#include <vector>

#include "include/ghc/filesystem.hpp"

namespace chromemedia {
namespace codec {

// EncodeWav for a batch: wav_data[i] -> encoded_features[i] (packets of stream i, oldest first).  packet_sizes (optional):
// (*packet_sizes)[i][h] = bytes hop h of stream i added (0: the empty packet of a DTX noise hop).
bool EncodeWavs(const std::vector<std::vector<int16_t>>& wav_data, int num_channels, int sample_rate_hz, int bitrate,
                bool enable_preprocessing, bool enable_dtx, const ghc::filesystem::path& model_path,
                std::vector<std::vector<uint8_t>>* encoded_features, int device = 0,
                std::vector<std::vector<int32_t>>* packet_sizes = nullptr);

// EncodeFile for a batch: wav_paths[i] -> output_paths[i].
bool EncodeFiles(const std::vector<ghc::filesystem::path>& wav_paths,
                 const std::vector<ghc::filesystem::path>& output_paths, int bitrate, bool enable_preprocessing,
                 bool enable_dtx, const ghc::filesystem::path& model_path, int device = 0);

// DecodeFeatures for a batch, no packet loss: packet_streams[i] (multiple of packet_size bytes) -> decoded_audio[i],
// at 16 kHz or, second form, at sample_rate_hz.
bool DecodeFeaturesBatch(const std::vector<std::vector<uint8_t>>& packet_streams, int packet_size,
                         const ghc::filesystem::path& model_path, std::vector<std::vector<int16_t>>* decoded_audio,
                         int device = 0);
bool DecodeFeaturesBatch(const std::vector<std::vector<uint8_t>>& packet_streams, int packet_size, int sample_rate_hz,
                         const ghc::filesystem::path& model_path, std::vector<std::vector<int16_t>>* decoded_audio,
                         int device = 0);

// ... with hops that carry no packet (DTX's empty packets, packets lost on the way): packet_sizes[i][h] = 0 or packet_size as
// EncodeWavs returns them, packet_streams[i] the non-empty packets concatenated.  Hop by hop through BatchLyraDecoder:
// SetEncodedPackets for the streams with a packet, DecodeSamples(one hop) for all.
bool DecodeFeaturesBatch(const std::vector<std::vector<uint8_t>>& packet_streams,
                         const std::vector<std::vector<int32_t>>& packet_sizes, int packet_size, int sample_rate_hz,
                         const ghc::filesystem::path& model_path, std::vector<std::vector<int16_t>>* decoded_audio,
                         int device = 0);

// DecodeFile for a batch: encoded_paths[i] (.lyra) -> output_paths[i] (16-bit mono WAV at sample_rate_hz).
bool DecodeFiles(const std::vector<ghc::filesystem::path>& encoded_paths,
                 const std::vector<ghc::filesystem::path>& output_paths, int sample_rate_hz, int bitrate,
                 const ghc::filesystem::path& model_path, int device = 0);

// ---- Time-parallel forms: long recordings at batch throughput --------------------------------------------------------
// The same results, byte for byte, as the functions above, through lyra_hip_encode_spans[_ext] / lyra_hip_decode_spans[_ext]
// (include/lyra_hip.h "Time-parallel spans"): every file is one span, cut into chunks that run side by side on up to
// num_lanes scratch streams of the context, each behind a discarded warm-up.  The hop-by-hop functions above advance one hop
// per blocking call -- one file, or the long tail of a batch of unequal files, is B = 1; these take a number of steps of about
// total hops / lanes + warm-up.  Lanes are capped so that a chunk is at least as long as its warm-up.
constexpr int kDefaultSpanLanes = 4096;
bool EncodeWavsTimeParallel(const std::vector<std::vector<int16_t>>& wav_data, int num_channels, int sample_rate_hz,
                            int bitrate, bool enable_preprocessing, bool enable_dtx,
                            const ghc::filesystem::path& model_path, std::vector<std::vector<uint8_t>>* encoded_features,
                            int num_lanes = kDefaultSpanLanes, int device = 0,
                            std::vector<std::vector<int32_t>>* packet_sizes = nullptr);
// ... with a bitrate per hop, LyraEncoder::set_bitrate between hops, through lyra_hip_encode_spans_mixed
// (include/lyra_hip_spans_mixed.h): bitrates[i][h] = 3200 / 6000 / 9200 for hop h of file i.  packet_sizes is part of the result:
// encoded_features[i] is the non-empty packets concatenated and cannot be cut into hops without them.
bool EncodeWavsTimeParallel(const std::vector<std::vector<int16_t>>& wav_data, int num_channels, int sample_rate_hz,
                            const std::vector<std::vector<int>>& bitrates, bool enable_preprocessing, bool enable_dtx,
                            const ghc::filesystem::path& model_path, std::vector<std::vector<uint8_t>>* encoded_features,
                            std::vector<std::vector<int32_t>>* packet_sizes, int num_lanes = kDefaultSpanLanes, int device = 0);
bool EncodeFilesTimeParallel(const std::vector<ghc::filesystem::path>& wav_paths,
                             const std::vector<ghc::filesystem::path>& output_paths, int bitrate, bool enable_preprocessing,
                             bool enable_dtx, const ghc::filesystem::path& model_path, int num_lanes = kDefaultSpanLanes,
                             int device = 0);
bool DecodeFeaturesTimeParallel(const std::vector<std::vector<uint8_t>>& packet_streams, int packet_size,
                                const ghc::filesystem::path& model_path, std::vector<std::vector<int16_t>>* decoded_audio,
                                int num_lanes = kDefaultSpanLanes, int device = 0);
bool DecodeFeaturesTimeParallel(const std::vector<std::vector<uint8_t>>& packet_streams, int packet_size, int sample_rate_hz,
                                const ghc::filesystem::path& model_path, std::vector<std::vector<int16_t>>* decoded_audio,
                                int num_lanes = kDefaultSpanLanes, int device = 0);
// ... with hops that carry no packet, through lyra_hip_decode_spans_lossy: the samples of the DecodeFeaturesBatch form that
// takes packet_sizes (what EncodeWavsTimeParallel(enable_dtx) returns; a loss trace has the same shape).
bool DecodeFeaturesTimeParallel(const std::vector<std::vector<uint8_t>>& packet_streams,
                                const std::vector<std::vector<int32_t>>& packet_sizes, int packet_size, int sample_rate_hz,
                                const ghc::filesystem::path& model_path, std::vector<std::vector<int16_t>>* decoded_audio,
                                int num_lanes = kDefaultSpanLanes, int device = 0);
// ... with every hop's size its own, as SetEncodedPacket reads it, through lyra_hip_decode_spans_lossy_mixed: packet_sizes[i][h]
// = 0 / 8 / 15 / 23, packet_streams[i] the non-empty packets concatenated (what the EncodeWavsTimeParallel form above returns).
bool DecodeFeaturesTimeParallel(const std::vector<std::vector<uint8_t>>& packet_streams,
                                const std::vector<std::vector<int32_t>>& packet_sizes, int sample_rate_hz,
                                const ghc::filesystem::path& model_path, std::vector<std::vector<int16_t>>* decoded_audio,
                                int num_lanes = kDefaultSpanLanes, int device = 0);
bool DecodeFilesTimeParallel(const std::vector<ghc::filesystem::path>& encoded_paths,
                             const std::vector<ghc::filesystem::path>& output_paths, int sample_rate_hz, int bitrate,
                             const ghc::filesystem::path& model_path, int num_lanes = kDefaultSpanLanes, int device = 0);

// ---- Time-parallel forms for files of ANY rate side by side ---------------------------------------------------------------------
// An archive of recordings at 8, 16, 32 and 48 kHz in ONE call per direction, through lyra_hip_encode_spans_packed /
// lyra_hip_decode_spans[_lossy]_packed (include/lyra_hip_spans_packed.h): every file is one span at its own rate, the files' samples
// lie back to back in one flat buffer and exactly those samples cross the bus.  sample_rates_hz holds one rate per file / stream.
// Per file the bytes are those of the functions above at that file's rate.  With enable_dtx each file's estimator runs at its own
// rate.  Lanes are capped as above, on the total number of hops.
bool EncodeWavsAnyRateTimeParallel(const std::vector<std::vector<int16_t>>& wav_data, const std::vector<int>& sample_rates_hz,
                                   int bitrate, bool enable_dtx, const ghc::filesystem::path& model_path,
                                   std::vector<std::vector<uint8_t>>* encoded_features,
                                   std::vector<std::vector<int32_t>>* packet_sizes, int num_lanes = kDefaultSpanLanes,
                                   int device = 0);
// ... with a bitrate per hop: bitrates[i][h] = 3200 / 6000 / 9200 for hop h of file i
bool EncodeWavsAnyRateTimeParallel(const std::vector<std::vector<int16_t>>& wav_data, const std::vector<int>& sample_rates_hz,
                                   const std::vector<std::vector<int>>& bitrates, bool enable_dtx,
                                   const ghc::filesystem::path& model_path, std::vector<std::vector<uint8_t>>* encoded_features,
                                   std::vector<std::vector<int32_t>>* packet_sizes, int num_lanes = kDefaultSpanLanes,
                                   int device = 0);
// packet_sizes[i][h] = 0 / 8 / 15 / 23, packet_streams[i] the non-empty packets concatenated (what the functions above return);
// decoded_audio[i] holds packet_sizes[i].size() hops at sample_rates_hz[i].  Streams whose hops all carry a packet of one size
// take the call without loss handling, which never blocks the host.
bool DecodeFeaturesAnyRateTimeParallel(const std::vector<std::vector<uint8_t>>& packet_streams,
                                       const std::vector<std::vector<int32_t>>& packet_sizes,
                                       const std::vector<int>& sample_rates_hz, const ghc::filesystem::path& model_path,
                                       std::vector<std::vector<int16_t>>* decoded_audio, int num_lanes = kDefaultSpanLanes,
                                       int device = 0);
// Whole files: the encode reads each WAV's own rate (mono, one of the four); the decode takes a rate per output file and cuts
// every .lyra file into packets of the bitrate's size.
bool EncodeFilesAnyRateTimeParallel(const std::vector<ghc::filesystem::path>& wav_paths,
                                    const std::vector<ghc::filesystem::path>& output_paths, int bitrate, bool enable_dtx,
                                    const ghc::filesystem::path& model_path, int num_lanes = kDefaultSpanLanes, int device = 0);
bool DecodeFilesAnyRateTimeParallel(const std::vector<ghc::filesystem::path>& encoded_paths,
                                    const std::vector<ghc::filesystem::path>& output_paths,
                                    const std::vector<int>& sample_rates_hz, int bitrate, const ghc::filesystem::path& model_path,
                                    int num_lanes = kDefaultSpanLanes, int device = 0);

// Minimal RIFF/WAVE PCM16 I/O (the reference uses audio_dsp's wav_util: Read16BitWavFileToVector /
// Write16BitWavFileFromVector).  False on anything but uncompressed 16-bit PCM.
bool ReadWav16(const ghc::filesystem::path& path, std::vector<int16_t>* samples, int* num_channels,
               int* sample_rate_hz);
bool WriteWav16(const ghc::filesystem::path& path, const std::vector<int16_t>& samples, int num_channels,
                int sample_rate_hz);

}  // namespace codec
}  // namespace chromemedia
#endif
