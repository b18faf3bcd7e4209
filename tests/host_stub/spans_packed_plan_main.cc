// spans_packed_plan_main.cc -- TEST INFRASTRUCTURE (tests/test_spans_packed_cpu.py): lyra_amd/csrc/spans_packed_plan.h behind a
// main of its own, built with -fsanitize=address,undefined and run directly.  Reads cases from stdin, one per line:
//   <n_spans> <n_ext> <use_offsets 0|1> then per span <n_frames> <rate> <offset>
// and prints per case: <layout total or -1> <check verdict: 0 accepted, else refused> <the bases used, if accepted>.
#include <cstdio>
#include <vector>

#include "../../lyra_amd/csrc/spans_packed_plan.h"

struct Span { int32_t stream_id; int32_t pad; int64_t first_frame, n_frames; };

int main() {
  int n = 0, use = 0;
  long long n_ext = 0;
  while (std::scanf("%d %lld %d", &n, &n_ext, &use) == 3) {
    std::vector<Span> spans((size_t)n);
    std::vector<int32_t> rates((size_t)n);
    std::vector<long long> given((size_t)n), base((size_t)n, 0);
    for (int s = 0; s < n; ++s) {
      long long frames = 0;
      int rate = 0;
      if (std::scanf("%lld %d %lld", &frames, &rate, &given[(size_t)s]) != 3) return 2;
      spans[(size_t)s] = Span{s, 0, 0, frames};
      rates[(size_t)s] = rate;
    }
    const long long total = lyra::spk::layout(spans.data(), n, rates.data(), base.data());
    int verdict = -1;
    if (use) base = given;
    if (use || total >= 0) verdict = lyra::spk::check(spans.data(), n, rates.data(), base.data(), n_ext);
    std::printf("%lld %d", total, verdict);
    for (int s = 0; verdict == 0 && s < n; ++s) std::printf(" %lld", base[(size_t)s]);
    std::printf("\n");
  }
  return 0;
}
