// Stand-alone driver for di_rank_record_bytes (csrc/contact_rank.hip) under AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/test_rank_record_host_sanitized.py builds both with
// -Xarch_host -fsanitize=address,undefined and runs this program; device code is not sanitized and
// nothing is launched: the function is host arithmetic). It walks every k of small shapes, the extreme
// sizes and every refusal, with an offsets array of exactly five words (a write past it is a heap
// overflow) and with NULL, and restates the layout from the header's comment.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/deepinteract_amd.h"

extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }  // the HIP runtime's own statics

static int failures = 0;
static void expect(long long got, long long want, const char* what) {
  if (got != want) {
    std::fprintf(stderr, "FAIL %s: got %lld, want %lld\n", what, got, want);
    ++failures;
  }
}

static void good(int32_t l1, int32_t l2, int32_t k) {
  for (int32_t with : {0, 1}) {
    std::vector<int64_t> off(5, 77);  // exactly five words on the heap
    const int64_t nb = di_rank_record_bytes(l1, l2, k, with, off.data());
    expect(di_rank_record_bytes(l1, l2, k, with, nullptr), nb, "NULL offsets: the same size");
    expect(nb > 0 && nb % 16 == 0, 1, "a positive multiple of 16");
    expect(off[0], 0, "ids");
    expect(off[1], 4ll * k, "scores");
    if (with) {
      const int64_t m = (12ll * k + 7) / 8 * 8;
      expect(off[2], 8ll * k, "hits");
      expect(off[3], m, "rank metrics");
      expect(off[4], m + (int64_t)sizeof(di_rank_metrics), "auc metrics");
      expect(nb, (m + (int64_t)sizeof(di_rank_metrics) + (int64_t)sizeof(di_auc_metrics) + 15) / 16 * 16, "bytes");
    } else {
      expect(off[2], -1, "no hits");
      expect(off[3], -1, "no rank metrics");
      expect(off[4], -1, "no auc metrics");
      expect(nb, (8ll * k + 15) / 16 * 16, "bytes without labels");
    }
  }
}

static void bad(int32_t l1, int32_t l2, int32_t k, int32_t with, int want, const char* what) {
  std::vector<int64_t> off(5, 77);
  expect(di_rank_record_bytes(l1, l2, k, with, off.data()), want, what);
  expect(di_rank_record_bytes(l1, l2, k, with, nullptr), want, what);
  for (int64_t o : off) expect(o, 77, "a refusal writes nothing");
}

int main() {
  for (int32_t l1 = 1; l1 <= 9; ++l1)
    for (int32_t l2 = 1; l2 <= 9; ++l2)
      for (int32_t k = 1; k <= l1 * l2; ++k) good(l1, l2, k);
  for (int32_t k : {1, 7, 1000, 4095, DI_RANK_MAX_K}) {
    good(4096, 4096, k);
    good(1, (1 << 29) - 1, k);
    good((1 << 29) - 1, 1, k);
    good(23170, 23170, k);  // 23170^2 = 536848900 < 2^29
  }
  good(1000, 1000, 1000);
  expect(di_rank_record_bytes(1000, 1000, 1000, 1, nullptr), 12112, "1000 x 1000 with labels");

  for (int32_t with : {0, 1}) {
    for (int32_t v : {0, -1, INT32_MIN}) {
      bad(v, 5, 1, with, DI_EINVAL, "l1 < 1");
      bad(5, v, 1, with, DI_EINVAL, "l2 < 1");
      bad(5, 5, v, with, DI_EINVAL, "k < 1");
      bad(v, v, v, with, DI_EINVAL, "everything < 1");
    }
    bad(5, 5, 26, with, DI_EINVAL, "k > l1 * l2");
    bad(1, 1, 2, with, DI_EINVAL, "k > l1 * l2 = 1");
    bad(10, 10, 5000, with, DI_EINVAL, "k > l1 * l2 comes before k > DI_RANK_MAX_K");
    bad(10, 10, INT32_MAX, with, DI_EINVAL, "k = INT32_MAX > l1 * l2");
    bad(100, 100, DI_RANK_MAX_K + 1, with, DI_ERANGE, "k > DI_RANK_MAX_K");
    bad(INT32_MAX, INT32_MAX, INT32_MAX, with, DI_ERANGE, "k = INT32_MAX");
    bad(1 << 15, 1 << 14, 10, with, DI_ERANGE, "l1 * l2 = 2^29");
    bad(1, 1 << 29, 10, with, DI_ERANGE, "l2 = 2^29");
    bad(INT32_MAX, INT32_MAX, 10, with, DI_ERANGE, "l1 * l2 near 2^62");
    bad(INT32_MAX, 1, 10, with, DI_ERANGE, "l1 = INT32_MAX");
  }
  for (int32_t with : {2, -1, INT32_MAX, INT32_MIN}) bad(5, 5, 5, with, DI_EINVAL, "with_labels other than 0 / 1");

  if (failures) return 1;
  std::puts("host_rank_record_san: ok");
  return 0;
}
