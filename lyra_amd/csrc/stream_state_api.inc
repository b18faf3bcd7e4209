// stream_state_api.inc -- part of api.hip: lyra_hip_export_streams / lyra_hip_import_streams, a stream's whole codec state
// as one relocatable blob (stream_blob.h) so a live stream can move to another id, context, GPU or process.  Control-plane
// calls with lyra_hip_reset_streams' ordering: the context is drained before the kernel and after it, so nothing is in
// flight while state is read or replaced; refused while a pipelined host request is outstanding (its begin() has enqueued
// work whose end() has not run).
#include "stream_blob.h"

static_assert(lyra::sb::SIDE_ENCODER == LYRA_HIP_STATE_ENCODER && lyra::sb::SIDE_DECODER == LYRA_HIP_STATE_DECODER, "side mask");
static_assert(lyra::sb::N_PIECES == lyra::st::R_COUNT + 3, "layout table");

namespace {

void blob_free(lyra_hip_ctx* c) {
  dfree(c->d_import_err, c->d_blobs);
  c->blob_cap = 0;
}

int blob_call_begin(lyra_hip_ctx* c, int B, const char* what) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if (pl_any_in_flight(c))
    return fail(c, LYRA_HIP_EINVAL, "%s: a pipelined request is outstanding (call its _end first)", what);
  for (int r = 0; r < st::R_COUNT; ++r)
    if (c->sm.bytes[r] != sb::region_bytes(r)) return fail(c, LYRA_HIP_EINVAL, "%s: region %d is not laid out as the blob's", what, r);
  return 0;
}

int blob_stage(lyra_hip_ctx* c, int B) {
  if (B <= c->blob_cap) return 0;
  dfree(c->d_blobs);
  c->blob_cap = 0;
  HIPCHK(c, dalloc(&c->d_blobs, (size_t)B * sb::BYTES));
  c->blob_cap = B;
  return 0;
}

// The staging of a large call (4096 streams: 350 MB) is given back when the call ends (the context is drained by then); a
// small one is kept for the next call.
void blob_stage_release(lyra_hip_ctx* c) {
  if ((size_t)c->blob_cap * sb::BYTES <= ((size_t)8 << 20)) return;
  dfree(c->d_blobs);
  c->blob_cap = 0;
}

// drained context in, drained context out
int export_run(lyra_hip_ctx* c, const int32_t* d_ids, int B, uint8_t* d_blobs) {
  int rc = sync_all(c);
  if (rc) return rc;
  hipLaunchKernelGGL(state_export_kernel, dim3(B), dim3(256), 0, c->se[0], d_ids, B, c->max_streams, c->sm,
                     (const float*)c->d_ds_ring, (const int16_t*)c->d_ds_gan, (const int16_t*)c->d_ds_cng, (unsigned)c->mode,
                     c->cng_seed, d_blobs);
  HIPCHK(c, hipGetLastError());
  return sync_all(c);
}

int import_run(lyra_hip_ctx* c, const int32_t* d_ids, int B, const uint8_t* d_blobs, unsigned sides) {
  int rc = sync_all(c);
  if (rc) return rc;
  if ((sides & LYRA_HIP_STATE_DECODER) && (rc = ds_ensure_streams(c))) return rc;
  if ((rc = err_word_ensure(c, &c->d_import_err))) return rc;
  hipLaunchKernelGGL(state_import_kernel, dim3(B), dim3(256), 0, c->se[0], d_ids, B, c->max_streams, c->sm, c->d_ds_ring,
                     c->d_ds_gan, c->d_ds_cng, (unsigned)c->mode, c->cng_seed, sides, d_blobs, c->d_import_err);
  HIPCHK(c, hipGetLastError());
  return sync_all(c);
}

int check_sides(lyra_hip_ctx* c, unsigned sides) {
  if (sides == 0 || (sides & ~(unsigned)(LYRA_HIP_STATE_ENCODER | LYRA_HIP_STATE_DECODER)))
    return fail(c, LYRA_HIP_EINVAL, "import_streams: sides %u is not a mask of LYRA_HIP_STATE_ENCODER | LYRA_HIP_STATE_DECODER", sides);
  return 0;
}

}  // namespace

extern "C" {

size_t lyra_hip_stream_blob_bytes(void) { return (size_t)sb::BYTES; }

int lyra_hip_export_streams_dev(lyra_hip_ctx* c, const int32_t* d_ids, int B, uint8_t* d_blobs) {
  int rc = blob_call_begin(c, B, "export_streams");
  if (rc) return rc;
  if (!d_ids || !d_blobs) return fail(c, LYRA_HIP_EINVAL, "export_streams: null pointer");
  if (reinterpret_cast<uintptr_t>(d_blobs) & 15) return fail(c, LYRA_HIP_EINVAL, "export_streams: d_blobs must be 16-byte aligned");
  DEVSCOPE(c);
  return export_run(c, d_ids, B, d_blobs);
}

int lyra_hip_import_streams_dev(lyra_hip_ctx* c, const int32_t* d_ids, int B, const uint8_t* d_blobs, unsigned sides) {
  int rc = blob_call_begin(c, B, "import_streams");
  if (rc) return rc;
  if ((rc = check_sides(c, sides))) return rc;
  if (!d_ids || !d_blobs) return fail(c, LYRA_HIP_EINVAL, "import_streams: null pointer");
  if (reinterpret_cast<uintptr_t>(d_blobs) & 15) return fail(c, LYRA_HIP_EINVAL, "import_streams: d_blobs must be 16-byte aligned");
  DEVSCOPE(c);
  return import_run(c, d_ids, B, d_blobs, sides);
}

int lyra_hip_export_streams(lyra_hip_ctx* c, const int32_t* ids, int B, uint8_t* blobs) {
  int rc = blob_call_begin(c, B, "export_streams");
  if (rc) return rc;
  if (!blobs) return fail(c, LYRA_HIP_EINVAL, "export_streams: null pointer");
  if ((rc = check_ids_host(c, ids, B))) return rc;
  DEVSCOPE(c);
  if ((rc = ensure_scratch(c, B))) return rc;
  if ((rc = blob_stage(c, B))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_ids, ids, (size_t)B * 4, hipMemcpyHostToDevice, c->se[0]));
  if ((rc = export_run(c, c->d_ids, B, c->d_blobs))) return rc;
  HIPCHK(c, hipMemcpy(blobs, c->d_blobs, (size_t)B * sb::BYTES, hipMemcpyDeviceToHost));
  blob_stage_release(c);
  return 0;
}

int lyra_hip_import_streams(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* blobs, unsigned sides) {
  int rc = blob_call_begin(c, B, "import_streams");
  if (rc) return rc;
  if ((rc = check_sides(c, sides))) return rc;
  if (!blobs) return fail(c, LYRA_HIP_EINVAL, "import_streams: null pointer");
  if ((rc = check_ids_host(c, ids, B))) return rc;
  for (int b = 0; b < B; ++b) {   // nothing is enqueued unless every row passes
    const int v = sb::validate(blobs + (size_t)b * sb::BYTES, (uint32_t)c->mode);
    if (v != sb::V_OK) return fail(c, LYRA_HIP_EINVAL, "import_streams: blob %d refused (stream_blob.h check %d)", b, v);
  }
  DEVSCOPE(c);
  if ((rc = ensure_scratch(c, B))) return rc;
  if ((rc = blob_stage(c, B))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_ids, ids, (size_t)B * 4, hipMemcpyHostToDevice, c->se[0]));
  HIPCHK(c, hipMemcpyAsync(c->d_blobs, blobs, (size_t)B * sb::BYTES, hipMemcpyHostToDevice, c->se[0]));
  rc = import_run(c, c->d_ids, B, c->d_blobs, sides);
  blob_stage_release(c);
  return rc;
}

long lyra_hip_import_errors(lyra_hip_ctx* c, int clear) {
  return read_error_counter(c, &lyra_hip_ctx::d_import_err, clear);
}

}  // extern "C"
