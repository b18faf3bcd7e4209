// stream_state_kernels.hip -- lyra_hip_export_streams / lyra_hip_import_streams (api.hip, stream_state_api.inc): a stream's
// state between its slots in the 12 regions (+ the by-id arrays of lyra_hip_decode_samples_dev) and one blob row
// (stream_blob.h).  One workgroup per row walks the regions as reset_kernel does; lane l moves bytes 16 l .. 16 l + 15 of
// every 4 KB step with one 16-byte load and one 16-byte store, so both sides are coalesced.  A row of id -1 (or an id
// outside the context) is skipped.  Nothing else may run on the context meanwhile (the host drains it before and after).
#include "kernels.h"
#include "stream_blob.h"

namespace lyra {

__device__ __forceinline__ i32x4 ld16(const uint8_t* p) { return *reinterpret_cast<const i32x4*>(p); }
__device__ __forceinline__ void st16(uint8_t* p, i32x4 v) { *reinterpret_cast<i32x4*>(p) = v; }

// blobs [B][sb::BYTES]; ring / gan / cng: the context's by-id arrays, or null (all three) when it never allocated them.
// ring slots that do not wait and hops that are not being read are exported as zero.
// The effective comfort-noise key seed ^ id ^ slot key goes into the header, zero into the payload's key word.
__global__ __launch_bounds__(256) void state_export_kernel(const int32_t* __restrict__ ids, int B, int max_streams, StateMap sm,
                                                            const float* __restrict__ ring, const int16_t* __restrict__ gan,
                                                            const int16_t* __restrict__ cng, unsigned mode,
                                                            unsigned long long seed, uint8_t* __restrict__ blobs) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= B) return;
  const int id = ids[b];
  if ((unsigned)id >= (unsigned)max_streams) return;   // (workgroup-uniform)
  uint8_t* blob = blobs + (size_t)b * sb::BYTES;
  if (tid < sb::HEADER_BYTES / 16) {
    const unsigned long long slot_key =
        *reinterpret_cast<const unsigned long long*>(sm.base[st::R_CNG] + (size_t)id * st::CNG_BYTES + st::C_KEY);
    uint32_t w[16];
    sb::header_words(mode, id, seed ^ (unsigned long long)(unsigned)id ^ slot_key, w);
    i32x4 q = (i32x4){0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k)   // (no runtime-indexed register array)
      if (tid == k) q = (i32x4){(int)w[4 * k], (int)w[4 * k + 1], (int)w[4 * k + 2], (int)w[4 * k + 3]};
    st16(blob + tid * 16, q);
  }
  uint8_t* dst = blob + sb::STATE_OFF;
#pragma unroll 1
  for (int r = 0; r < st::R_COUNT; ++r) {
    const int bytes = sm.bytes[r];
    const uint8_t* src = sm.base[r] + (size_t)id * bytes;
    for (int o = tid * 16; o < bytes; o += 256 * 16) {
      i32x4 q = ld16(src + o);
      if (r == st::R_CNG && o == st::C_KEY) { q[0] = 0; q[1] = 0; }
      st16(dst + o, q);
    }
    dst += bytes;
  }
  // the decode-samples section: 64 + 40 + 40 lanes, each array on wavefronts of its own.  Only what the stream's counters
  // call live is exported -- the waiting ring slots, a hop that is being read -- and zero for the rest, so a blob does not
  // depend on what earlier streams of the slot left in the arrays.
  const DsState s = *reinterpret_cast<const DsState*>(sm.base[st::R_CNG] + (size_t)id * st::CNG_BYTES + DS_STATE);
  const i32x4 zero = (i32x4){0, 0, 0, 0};
  if (tid < sb::DS_RING_BYTES / 16) {
    const bool live = ring && (((tid >> 4) - s.head) & (DS_FIFO_DEPTH - 1)) < s.wait;
    st16(blob + sb::DS_RING_OFF + tid * 16,
         live ? ld16(reinterpret_cast<const uint8_t*>(ring) + (size_t)id * sb::DS_RING_BYTES + tid * 16) : zero);
  }
  const int t1 = tid - 64, t2 = tid - 128;
  if (t1 >= 0 && t1 < sb::DS_HOP_BYTES / 16)
    st16(blob + sb::DS_GAN_OFF + t1 * 16,
         gan && s.gpos ? ld16(reinterpret_cast<const uint8_t*>(gan) + (size_t)id * sb::DS_HOP_BYTES + t1 * 16) : zero);
  if (t2 >= 0 && t2 < sb::DS_HOP_BYTES / 16)
    st16(blob + sb::DS_CNG_OFF + t2 * 16,
         cng && s.cpos ? ld16(reinterpret_cast<const uint8_t*>(cng) + (size_t)id * sb::DS_HOP_BYTES + t2 * 16) : zero);
}
static_assert((DS_FIFO_DEPTH & (DS_FIFO_DEPTH - 1)) == 0, "ring slot arithmetic above");
static_assert(st::C_KEY % 16 == 0 && sb::DS_RING_BYTES / 16 <= 64 && sb::DS_HOP_BYTES / 16 <= 64, "lane assignment above");

// The row is judged first -- sb::validate on the header and on every integer a kernel forms an address or a trip count
// from, by one lane, then one workgroup-uniform decision -- and only then written: a rejected row leaves the target stream
// untouched and adds one to *err.  Only the regions of the sides asked for are written (sb::region_side; the
// decode-samples arrays belong to the decoder side and are allocated by the host before the launch when it is asked for).
// The key word of the R_CNG slot becomes header key ^ seed ^ id: the stream keeps its effective comfort-noise key.
__global__ __launch_bounds__(256) void state_import_kernel(const int32_t* __restrict__ ids, int B, int max_streams, StateMap sm,
                                                            float* __restrict__ ring, int16_t* __restrict__ gan,
                                                            int16_t* __restrict__ cng, unsigned mode, unsigned long long seed,
                                                            unsigned sides, const uint8_t* __restrict__ blobs,
                                                            unsigned* __restrict__ err) {
  __shared__ int sh_verdict;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= B) return;
  const int id = ids[b];
  if (id == -1) return;                                  // (workgroup-uniform)
  const uint8_t* blob = blobs + (size_t)b * sb::BYTES;
  if (tid == 0) sh_verdict = (unsigned)id >= (unsigned)max_streams ? -1 : sb::validate(blob, mode);
  __syncthreads();
  if (sh_verdict != sb::V_OK) {
    if (tid == 0) atomicAdd(err, 1u);
    return;
  }
  const unsigned long long key = sb::header_key(blob) ^ seed ^ (unsigned long long)(unsigned)id;
  const uint8_t* src = blob + sb::STATE_OFF;
#pragma unroll 1
  for (int r = 0; r < st::R_COUNT; ++r) {
    const int bytes = sm.bytes[r];
    if (sb::region_side(r) & sides) {
      uint8_t* dst = sm.base[r] + (size_t)id * bytes;
      for (int o = tid * 16; o < bytes; o += 256 * 16) {
        i32x4 q = ld16(src + o);
        if (r == st::R_CNG && o == st::C_KEY) { q[0] = (int)(unsigned)key; q[1] = (int)(unsigned)(key >> 32); }
        st16(dst + o, q);
      }
    }
    src += bytes;
  }
  if (!(sides & sb::SIDE_DECODER)) return;
  if (tid < sb::DS_RING_BYTES / 16)
    st16(reinterpret_cast<uint8_t*>(ring) + (size_t)id * sb::DS_RING_BYTES + tid * 16, ld16(blob + sb::DS_RING_OFF + tid * 16));
  const int t1 = tid - 64, t2 = tid - 128;
  if (t1 >= 0 && t1 < sb::DS_HOP_BYTES / 16)
    st16(reinterpret_cast<uint8_t*>(gan) + (size_t)id * sb::DS_HOP_BYTES + t1 * 16, ld16(blob + sb::DS_GAN_OFF + t1 * 16));
  if (t2 >= 0 && t2 < sb::DS_HOP_BYTES / 16)
    st16(reinterpret_cast<uint8_t*>(cng) + (size_t)id * sb::DS_HOP_BYTES + t2 * 16, ld16(blob + sb::DS_CNG_OFF + t2 * 16));
}

}  // namespace lyra
