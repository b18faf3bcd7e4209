// fake_encode_streams_abi.cc -- TEST INFRASTRUCTURE: a CPU stand-in for the three calls of include/lyra_hip_encode_streams.h,
// linked next to tests/host_stub/fake_lyra_hip_codec.cc (which has every other entry point the host classes use and stays as
// it is).  It records what each begin() received and answers with integer formulas of the row's own samples, so that a row
// read at the wrong packed offset, with the wrong bit count or for the wrong stream changes the packets.  Never linked into
// the product.
#include <cstdint>
#include <cstdlib>
#include <deque>
#include <vector>

#include "fake_encode_streams_abi.h"

std::vector<FakeStreamsCall> g_fake_streams_calls;
int g_fake_streams_ends = 0;

namespace {
struct Result { std::vector<uint8_t> pk; std::vector<int32_t> len; };
std::deque<Result> g_queue;
}  // namespace

extern "C" {

int lyra_hip_encode_streams_dev(lyra_hip_ctx*, const int32_t*, int, const int16_t*, long, const int32_t*, const int32_t*,
                                const int32_t*, const int32_t*, uint8_t*, int32_t*) {
  return -1;   // (device buffers: nothing a host class calls)
}

int lyra_hip_encode_streams_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const int16_t* pcm, const int32_t* rates,
                                  const int32_t* bits, const int32_t* dtx) {
  if (!c || !ids || B <= 0 || !pcm || !rates || !bits || g_queue.size() >= 2) return -1;
  FakeStreamsCall call;
  call.B = B;
  call.dtx_null = dtx == nullptr;
  Result r;
  r.pk.assign(static_cast<size_t>(B) * 23, 0);
  r.len.assign(B, 0);
  size_t off = 0;
  for (int b = 0; b < B; ++b) {
    const int n = rates[b] / 50;
    call.ids.push_back(ids[b]);
    call.rates.push_back(rates[b]);
    call.bits.push_back(bits[b]);
    call.dtx.push_back(dtx ? dtx[b] : 0);
    call.offsets.push_back(static_cast<long>(off));
    call.first.push_back(pcm[off]);
    call.last.push_back(pcm[off + n - 1]);
    bool quiet = true;
    for (int i = 0; i < n; ++i) quiet = quiet && std::abs(static_cast<int>(pcm[off + i])) < 64;
    if (!(dtx && dtx[b] && quiet)) {   // a DTX stream's quiet hop: the empty packet
      const int nbytes = (bits[b] + 7) / 8;
      r.len[b] = nbytes;
      for (int j = 0; j < nbytes; ++j)
        r.pk[static_cast<size_t>(b) * 23 + j] = static_cast<uint8_t>(pcm[off + (j * 7) % n] + 31 * j + ids[b] + bits[b]);
    }
    off += n;
  }
  call.total = static_cast<long>(off);
  g_fake_streams_calls.push_back(call);
  g_queue.push_back(r);
  return 0;
}

int lyra_hip_encode_streams_end(lyra_hip_ctx* c, uint8_t* packets, int32_t* packet_bytes) {
  if (!c || !packets || !packet_bytes || g_queue.empty()) return -1;
  const Result& r = g_queue.front();
  for (size_t i = 0; i < r.pk.size(); ++i) packets[i] = r.pk[i];
  for (size_t i = 0; i < r.len.size(); ++i) packet_bytes[i] = r.len[i];
  g_queue.pop_front();
  ++g_fake_streams_ends;
  return 0;
}

}  // extern "C"
