// speakers_api.inc -- part of api.hip, behind bridge_api.inc: the conference bridge with loudest-N selection
// (include/lyra_hip_speakers.h).  The tick and the two-deep host form are those of bridge_api.inc (brg_tick_impl,
// brg_begin_impl: one body for both kinds of mix, the same slots and in-flight counters), with max_speakers >= 1; what is new
// here is the mix itself -- three kernels on se[0] (speakers_kernels.hip) -- its scratch, and the end() that also delivers
// levels and speaker flags.
#include "../../include/lyra_hip_speakers.h"

static_assert(LYRA_HIP_SPEAKERS_SKIP_COMFORT_NOISE == LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE, "one flag word for both ticks");
static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(unsigned long long) == 8, "the kernels' 64-bit words");

namespace {

void spk_free_bufs(lyra_hip_ctx* c) {
  for (int i = 0; i < 2; ++i) dfree(c->d_spk_list[i], c->d_spk_pos_room[i], c->d_spk_keys[i], c->d_spk_levels[i], c->d_spk_flags[i]);
  c->spk_cap = 0;
}
void spk_free(lyra_hip_ctx* c) { spk_free_bufs(c); }

// Speaker lists [n_rooms][8], pos_room and keys [n_members], and the levels / flags of a call that passes none: all sized by
// B (n_rooms, n_members <= B).  Two sets by lossy-call parity, like d_brg_mix; called before anything is enqueued.
int spk_ensure(lyra_hip_ctx* c, int B) {
  if (B <= c->spk_cap) return 0;
  int rc = sync_all(c);   // (the buffers of the calls in flight)
  if (rc) return rc;
  spk_free_bufs(c);
  for (int i = 0; i < 2; ++i) {
    HIPCHK(c, dalloc(&c->d_spk_list[i], (size_t)B * LYRA_HIP_SPEAKERS_MAX));
    HIPCHK(c, dalloc(&c->d_spk_pos_room[i], (size_t)B));
    HIPCHK(c, dalloc(&c->d_spk_keys[i], (size_t)B));
    HIPCHK(c, dalloc(&c->d_spk_levels[i], (size_t)B));
    HIPCHK(c, dalloc(&c->d_spk_flags[i], (size_t)B));
  }
  c->spk_cap = B;
  return 0;
}

// levels over all B rows (which also clears the mix, the flags and pos_room), then one wavefront per room, then one per eight
// positions of the index; on se[0].  spk_ensure(c, B) has run.
int spk_mix_launch(lyra_hip_ctx* c, const int16_t* d_pcm16, int B, const int32_t* d_order, const int32_t* d_room_start,
                   int n_rooms, int n_members, const int32_t* d_muted, const int32_t* d_is_cn, int max_speakers, int16_t* d_mix,
                   int64_t* d_levels, int32_t* d_is_speaker, int set) {
  long long* levels = reinterpret_cast<long long*>(d_levels ? d_levels : c->d_spk_levels[set]);
  int32_t* flags = d_is_speaker ? d_is_speaker : c->d_spk_flags[set];
  int32_t* pos_room = c->d_spk_pos_room[set];
  hipLaunchKernelGGL(speakers_level_kernel, dim3(cdiv(B, 4)), dim3(256), 0, c->se[0], d_pcm16, B, levels, d_mix, flags, pos_room,
                     n_members, (int32_t*)nullptr, (int32_t*)nullptr);
  HIPCHK(c, hipGetLastError());
  if (n_rooms > 0 && n_members > 0) {
    hipLaunchKernelGGL(speakers_select_kernel, dim3(cdiv(n_rooms, 4)), dim3(256), 0, c->se[0], levels, B, d_order, d_room_start,
                       n_rooms, n_members, d_muted, d_is_cn, max_speakers, c->d_spk_keys[set], c->d_spk_list[set], pos_room, flags,
                       c->d_bridge_err);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(speakers_mix_kernel, dim3(cdiv(n_members, 32)), dim3(256), 0, c->se[0], d_pcm16, B, d_order, n_members,
                       pos_room, n_rooms, c->d_spk_list[set], d_mix);
    HIPCHK(c, hipGetLastError());
  }
  return 0;
}

int spk_check_n(lyra_hip_ctx* c, const char* what, int max_speakers) {
  if (max_speakers < 1 || max_speakers > LYRA_HIP_SPEAKERS_MAX)
    return fail(c, LYRA_HIP_EINVAL, "%s: max_speakers %d outside 1..%d", what, max_speakers, LYRA_HIP_SPEAKERS_MAX);
  return 0;
}

}  // namespace

extern "C" {

int lyra_hip_speakers_mix_dev(lyra_hip_ctx* c, const int16_t* d_pcm16, int B, const int32_t* d_order, const int32_t* d_room_start,
                              int n_rooms, int n_members, const int32_t* d_muted, const int32_t* d_is_comfort_noise,
                              int max_speakers, int16_t* d_mix, int64_t* d_levels, int32_t* d_is_speaker) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if (!d_pcm16 || !d_mix) return fail(c, LYRA_HIP_EINVAL, "speakers_mix: null pointer");
  if ((rc = brg_check_index(c, "speakers_mix", B, d_order, d_room_start, n_rooms, n_members))) return rc;
  if (brg_misaligned(d_pcm16) || brg_misaligned(d_mix) || d_pcm16 == d_mix)
    return fail(c, LYRA_HIP_EINVAL, "speakers_mix: d_pcm16 and d_mix must be 16-byte aligned and distinct");
  if ((reinterpret_cast<uintptr_t>(d_levels) & 7u) != 0) return fail(c, LYRA_HIP_EINVAL, "speakers_mix: d_levels must be 8-byte aligned");
  if ((rc = spk_check_n(c, "speakers_mix", max_speakers))) return rc;
  DEVSCOPE(c);
  if ((rc = brg_ensure_mix(c))) return rc;
  if ((rc = spk_ensure(c, B))) return rc;
  if ((rc = enc_side_begin(c, 0))) return rc;
  rc = spk_mix_launch(c, d_pcm16, B, d_order, d_room_start, n_rooms, n_members, d_muted, d_is_comfort_noise, max_speakers, d_mix,
                      d_levels, d_is_speaker, (int)(c->n_lossy_calls & 1));
  if (!rc) rc = enc_side_done(c, 0);
  return rc;
}

int lyra_hip_speakers_tick_dev(lyra_hip_ctx* c, const lyra_hip_speakers_tick* S) {
  if (!c) return LYRA_HIP_EINVAL;
  if (!S) return fail(c, LYRA_HIP_EINVAL, "speakers_tick: null pointer");
  int rc = spk_check_n(c, "speakers_tick", S->max_speakers);
  if (rc) return rc;
  if ((reinterpret_cast<uintptr_t>(S->d_levels) & 7u) != 0)
    return fail(c, LYRA_HIP_EINVAL, "speakers_tick: d_levels must be 8-byte aligned");
  lyra_hip_bridge_tick T = {};   // the leading fields, one by one: the two structs are separate types
  T.d_stream_ids = S->d_stream_ids;
  T.B = S->B;
  T.d_packets = S->d_packets;
  T.d_packet_bytes = S->d_packet_bytes;
  T.d_order = S->d_order;
  T.d_room_start = S->d_room_start;
  T.n_rooms = S->n_rooms;
  T.n_members = S->n_members;
  T.d_muted = S->d_muted;
  T.flags = S->flags;
  T.d_num_bits = S->d_num_bits;
  T.d_dtx = S->d_dtx;
  T.d_out_packets = S->d_out_packets;
  T.d_out_packet_bytes = S->d_out_packet_bytes;
  T.d_pcm16 = S->d_pcm16;
  T.d_mix = S->d_mix;
  T.d_is_noise = S->d_is_noise;
  T.d_is_comfort_noise = S->d_is_comfort_noise;
  return brg_tick_impl(c, "speakers_tick", &T, S->max_speakers, S->d_levels, S->d_is_speaker);
}

int lyra_hip_speakers_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets, const int32_t* packet_bytes,
                            const int32_t* rooms, const int32_t* muted, unsigned flags, const int32_t* num_bits,
                            const int32_t* dtx, int max_speakers) {
  if (!c) return LYRA_HIP_EINVAL;
  int rc = spk_check_n(c, "speakers_begin", max_speakers);
  if (rc) return rc;
  return brg_begin_impl(c, "speakers_begin", ids, B, packets, packet_bytes, rooms, muted, flags, num_bits, dtx, max_speakers);
}

int lyra_hip_speakers_end(lyra_hip_ctx* c, uint8_t* out_packets, int32_t* out_packet_bytes, int32_t* is_noise,
                          int32_t* is_comfort_noise, int64_t* levels, int32_t* is_speaker) {
  if (!c) return LYRA_HIP_EINVAL;
  if (!c->brg_host || c->pl_ended[PL_BRIDGE] == c->pl_begun[PL_BRIDGE]) return fail(c, LYRA_HIP_EINVAL, "speakers_end: no tick in flight");
  BrgSlot& S = static_cast<BrgHost*>(c->brg_host)->slot[c->pl_ended[PL_BRIDGE] & 1];
  if (!S.max_speakers) return fail(c, LYRA_HIP_EINVAL, "speakers_end: the oldest tick was begun by the full-mix begin()");
  if (S.shared) return fail(c, LYRA_HIP_EINVAL, "speakers_end: the oldest tick was begun by lyra_hip_shared_begin");
  if (!out_packets || !out_packet_bytes) return fail(c, LYRA_HIP_EINVAL, "speakers_end: null pointer");
  DEVSCOPE(c);
  c->pl_ended[PL_BRIDGE]++;                  // whatever happens below, the slot is given back
  HIPCHK(c, hipEventSynchronize(S.ev_done));
  const size_t n = (size_t)S.B;
  std::memcpy(out_packet_bytes, S.h_out, n * 4);
  if (is_noise) std::memcpy(is_noise, S.h_out + n * 4, n * 4);
  if (is_comfort_noise) std::memcpy(is_comfort_noise, S.h_out + 2 * n * 4, n * 4);
  if (is_speaker) std::memcpy(is_speaker, S.h_out + 3 * n * 4, n * 4);
  if (levels) std::memcpy(levels, S.h_out + 4 * n * 4, n * 8);
  std::memcpy(out_packets, S.h_out + kSpkOutWords * n * 4, n * LYRA_HIP_MAX_PACKET_BYTES);
  return 0;
}

}  // extern "C"
