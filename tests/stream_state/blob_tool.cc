// blob_tool.cc -- test helper compiled by tests/test_stream_state_cpu.py against lyra_amd/csrc/stream_blob.h with a plain
// C++ compiler:  layout            prints the blob's layout table and the constants the test needs, as JSON
//                reset FILE MODE [Z x 7]  writes a blob built from the reset values (a fresh stream, source id 0, key 0); with the
//                                  seven zero points of the int8 histories (E_R2_1, E_R2_2, E_D2, E_BOTT, D_R0_0, D_R0_1,
//                                  D_R0_2) those hold them, as after lyra_hip_reset_streams; without, zero
//                validate FILE MODE  prints sb::validate's verdict of every blob in FILE, one per line
//                tensors           prints the offset of every tensor of the six stage regions and of M_PREV inside its region's
//                                  slot (state_layout.h), as JSON -- tests/state_bridge.py
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stream_blob.h"

using namespace lyra;

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "layout")) {
    printf("{\"bytes\": %d, \"header_bytes\": %d, \"state_bytes\": %d, \"section_bytes\": %d, \"ds_off\": %d,\n", sb::BYTES,
           sb::HEADER_BYTES, st::BYTES, sb::DS_SECTION_BYTES, sb::DS_OFF);
    printf(" \"magic\": %u, \"version\": %u, \"fingerprint\": %u, \"model\": %u, \"h_end\": %d,\n", sb::MAGIC, sb::VERSION,
           sb::FINGERPRINT, sb::MODEL_VERSION, sb::H_END);
    printf(" \"h\": {\"magic\": %d, \"version\": %d, \"bytes\": %d, \"fingerprint\": %d, \"mode\": %d, \"model\": %d, \"src_id\": %d, "
           "\"zero\": %d, \"key\": %d},\n", sb::H_MAGIC, sb::H_VERSION, sb::H_BYTES, sb::H_FINGERPRINT, sb::H_MODE, sb::H_MODEL,
           sb::H_SRC_ID, sb::H_ZERO, sb::H_KEY);
    printf(" \"phase\": %d, \"phase_mod\": %d, \"n_init\": %d, \"n_hops\": %d, \"n_is_noise\": %d, \"rs_in_pos\": %d, "
           "\"lossy_ctl\": %d, \"ds_state\": %d, \"c_key\": %d, \"c_ola\": %d, \"fifo\": %d, \"noise_hops_max\": %d,\n", st::PHASE,
           st::PHASE_MOD, st::N_INIT, st::N_HOPS, st::N_IS_NOISE, st::RS_IN_POS, LOSSY_CTL, DS_STATE, st::C_KEY, st::C_OLA,
           DS_FIFO_DEPTH, sb::NOISE_HOPS_MAX);
    printf(" \"region_bytes\": [");
    for (int r = 0; r < st::R_COUNT; ++r) printf("%s%d", r ? ", " : "", st::REGION_BYTES[r]);
    printf("],\n \"region_side\": [");
    for (int r = 0; r < st::R_COUNT; ++r) printf("%s%u", r ? ", " : "", sb::region_side(r));
    printf("],\n \"pieces\": [");
    for (int i = 0; i < sb::N_PIECES; ++i) printf("%s[%d, %d]", i ? ", " : "", sb::piece(i).off, sb::piece(i).bytes);
    printf("]}\n");
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "tensors")) {
#define T(name) printf("%s\"" #name "\": %d", first++ ? ", " : "{", st::name)
    int first = 0;
    T(E_FIRST); T(E_R0_0); T(E_R0_1); T(E_R0_2); T(E_D0); T(E_R1_0); T(E_R1_1); T(E_R1_2); T(E_D1); T(E_R2_0); T(E_R2_1);
    T(E_R2_2); T(E_D2); T(E_BOTT); T(D_HEAD); T(D_UP0); T(D_R0_0); T(D_R0_1); T(D_R0_2); T(D_UP1); T(D_R1_0); T(D_R1_1);
    T(D_R1_2); T(D_UP2); T(D_R2_0); T(D_R2_1); T(D_R2_2); T(D_UP3); T(M_PREV); T(PHASE); T(PHASE_MOD); T(HDR);
#undef T
    printf("}\n");
    return 0;
  }
  if ((argc == 4 || argc == 11) && !strcmp(argv[1], "reset")) {
    std::vector<uint8_t> b(sb::BYTES, 0);
    uint32_t w[16];
    sb::header_words((uint32_t)atoi(argv[3]), 0, 0, w);
    memcpy(b.data(), w, sizeof w);
    // (int8 histories hold their tensors' zero points after a reset: payload validate() does not look at)
    if (argc == 11) {
      const int reg[7] = {st::R_E2, st::R_E2, st::R_E2, st::R_E2, st::R_D0, st::R_D0, st::R_D0};
      const int lo[7] = {st::E_R2_1, st::E_R2_2, st::E_D2, st::E_BOTT, st::D_R0_0, st::D_R0_1, st::D_R0_2};
      const int hi[7] = {st::E_R2_2, st::E_D2, st::E_BOTT, st::E_BOTT + 2 * 512, st::D_R0_1, st::D_R0_2, st::D_UP1};
      for (int i = 0; i < 7; ++i) memset(b.data() + sb::region_off(reg[i]) + lo[i], (int8_t)atoi(argv[4 + i]), hi[i] - lo[i]);
    }
    sb::put32(b.data() + sb::region_off(st::R_NOISE_E) + st::N_IS_NOISE, 1);
    sb::put32(b.data() + sb::region_off(st::R_NOISE_D) + st::N_IS_NOISE, 1);
    FILE* f = fopen(argv[2], "wb");
    if (!f || fwrite(b.data(), 1, b.size(), f) != b.size()) return 2;
    fclose(f);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "validate")) {
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<uint8_t> b(sb::BYTES);
    while (fread(b.data(), 1, b.size(), f) == b.size()) printf("%d\n", sb::validate(b.data(), (uint32_t)atoi(argv[3])));
    fclose(f);
    return 0;
  }
  return 1;
}
