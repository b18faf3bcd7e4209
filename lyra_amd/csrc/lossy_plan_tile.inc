// lossy_plan_tile.inc -- part of lossy_kernels.hip: the body of lossy_plan_kernel and lossy_plan_mixed_kernel, included
// inside each kernel (a shared __device__ function changes the code of the shipped kernel).  The includer defines
// `constexpr bool MIXED`, `nbytes` and `bytes_from_bits` next to the kernel's own arguments.
  __shared__ int rx[256];
  const int tid = threadIdx.x, b0 = blockIdx.x * 256, b = b0 + tid;
  if (b < B) {
    const int id = ids[b];
    bool r = true;
    if (MIXED) {
      const int pb = mixed_bytes(pkt_bytes[b], bytes_from_bits);
      r = mixed_received(pb);
      if (pb != 0 && !r) atomicAdd(err, 1u);
    } else if (pkt_bytes) {
      const int pb = pkt_bytes[b];
      r = pb == nbytes;
      if (pb != 0 && pb != nbytes) atomicAdd(err, 1u);
    }
    if (rx_ring_row) r = r && rx_ring_row[b] != 0;
    uint32_t* ctl = reinterpret_cast<uint32_t*>(cng_state + (size_t)id * st::CNG_BYTES + LOSSY_CTL);
    const LossyTick t = lossy_tick(*ctl, r);
    *ctl = t.ctl;
    gen_ids[b] = t.run_gen ? id : -1;
    cng_ids[b] = t.run_cng ? id : -1;
    est_ids[b] = t.feed_est ? id : -1;
    info[b] = lossy_info(t);
    rx[tid] = r ? 1 : 0;
  } else {
    rx[tid] = 1;
  }
  __syncthreads();
  const int rows = min(256, B - b0);
  for (int i = tid; i < rows * 64; i += 256)
    if (!rx[i >> 6]) feats[(size_t)b0 * 64 + i] = 0.f;
