// speakers_api.inc -- part of api.hip, in front of bridge_api.inc: the loudest-N selection of the conference bridge
// (include/lyra_hip_speakers.h).  What is here is the mix itself -- three kernels on se[0] (speakers_kernels.hip) -- and its
// scratch.  The tick, the two-deep host form and the entry points are those of bridge_api.inc (brg_tick_impl, brg_begin_impl,
// brg_end_impl, brg_mix_call: one body for every kind of mix, the same slots and in-flight counters), with max_speakers >= 1.
#include "../../include/lyra_hip_bridge.h"
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
