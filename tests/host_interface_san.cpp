// Stand-alone driver for the host side of csrc/contact_interface.hip under AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/test_interface_host_sanitized.py builds both with
// -Xarch_host -fsanitize=address,undefined and runs this program; device code is not sanitized and
// nothing is launched: every call here is refused, or is the *_check form, before any launch).
// It walks the validation and the size / offset arithmetic of di_interface_work_bytes and
// di_interface_labels_batch(_check) with tables of exactly `count` items up to DI_BATCH_MAX, extreme
// sizes and cutoffs, and dummy pointers that are never dereferenced.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
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

int main() {
  void* const P = reinterpret_cast<void*>(16 * 1024);  // 16-B aligned, never dereferenced
  const int32_t shapes[][4] = {{1, 1, 1, 1},          {3, 5, 20, 40},         {145, 145, 1076, 1076},
                               {7, 400, 90, 5000},    {4096, 4096, 60000, 60000},
                               {1, (1 << 29) - 1, 1, (1 << 24) - 1},          {(1 << 29) - 1, 1, (1 << 24) - 1, 1}};
  const int nshapes = sizeof(shapes) / sizeof(shapes[0]);
  const float inf = std::numeric_limits<float>::infinity();

  auto make = [&](int count) {
    std::vector<di_interface_item> v(count);   // exactly count items: a read past the table is a heap overflow
    for (int i = 0; i < count; ++i) {
      di_interface_item it = {};
      it.xyz0 = it.xyz1 = reinterpret_cast<const float*>(P);
      it.res_off0 = it.res_off1 = reinterpret_cast<const int32_t*>(P);
      it.labels = reinterpret_cast<uint8_t*>(P);
      it.l1 = shapes[i % nshapes][0], it.l2 = shapes[i % nshapes][1];
      it.a0 = shapes[i % nshapes][2], it.a1 = shapes[i % nshapes][3];
      v[i] = it;
    }
    return v;
  };
  auto* dev = reinterpret_cast<const di_interface_item*>(P);

  for (int count : {1, 2, 7, 1023, DI_BATCH_MAX}) {
    auto v = make(count);
    const int64_t nb = di_interface_work_bytes(v.data(), count);
    expect(nb > 0 && nb % 16 == 0, 1, "work bytes");
    int64_t at = (int64_t)count * 16;
    for (int i = 0; i < count; ++i) {
      expect(v[i].work_off, at, "work_off");
      at += ((int64_t)v[i].l1 + v[i].l2) * 16;
    }
    expect(nb, at, "total");
    expect(di_interface_labels_batch_check(v.data(), dev, count, 6.0f, P), DI_OK, "check");
    expect(di_interface_labels_batch_check(v.data(), dev, count, std::numeric_limits<float>::max(), P), DI_OK,
           "the largest finite cutoff");
    expect(di_interface_labels_batch_check(v.data(), dev, count, std::numeric_limits<float>::denorm_min(), P), DI_OK,
           "the smallest positive cutoff");
    for (float bad : {0.0f, -0.0f, -6.0f, inf, -inf, std::nanf("")})
      expect(di_interface_labels_batch(v.data(), dev, count, bad, P, nullptr), DI_EINVAL, "bad cutoff");
    for (uintptr_t delta : {1u, 4u, 8u, 15u})
      expect(di_interface_labels_batch(v.data(), dev, count, 6.0f, reinterpret_cast<char*>(P) + delta, nullptr),
             DI_EINVAL, "misaligned work");

    di_interface_item& it = v[count - 1];
    const di_interface_item keep = it;
    it.work_off += 16;
    expect(di_interface_labels_batch(v.data(), dev, count, 6.0f, P, nullptr), DI_EINVAL, "stale work_off");
    it = keep, it.work_off = INT64_MAX;
    expect(di_interface_labels_batch(v.data(), dev, count, 6.0f, P, nullptr), DI_EINVAL, "work_off = INT64_MAX");
    it = keep, it.xyz0 = reinterpret_cast<const float*>(reinterpret_cast<char*>(P) + 2);
    expect(di_interface_labels_batch(v.data(), dev, count, 6.0f, P, nullptr), DI_EINVAL, "misaligned xyz0");
    it = keep, it.res_off1 = reinterpret_cast<const int32_t*>(reinterpret_cast<char*>(P) + 1);
    expect(di_interface_labels_batch(v.data(), dev, count, 6.0f, P, nullptr), DI_EINVAL, "misaligned res_off1");
    it = keep, it.labels = nullptr;
    expect(di_interface_labels_batch(v.data(), dev, count, 6.0f, P, nullptr), DI_EINVAL, "NULL labels");
    it = keep, it.xyz1 = nullptr;
    expect(di_interface_labels_batch(v.data(), dev, count, 6.0f, P, nullptr), DI_EINVAL, "NULL xyz1");
    for (int32_t bad : {0, -1, INT32_MIN}) {
      it = keep, it.l1 = bad;
      expect(di_interface_labels_batch(v.data(), dev, count, 6.0f, P, nullptr), DI_EINVAL, "l1 < 1");
      expect(di_interface_work_bytes(v.data(), count), DI_EINVAL, "work bytes, l1 < 1");
      it = keep, it.a1 = bad;
      expect(di_interface_labels_batch(v.data(), dev, count, 6.0f, P, nullptr), DI_EINVAL, "a1 < 1");
    }
    it = keep, it.l1 = INT32_MAX, it.l2 = INT32_MAX;
    expect(di_interface_labels_batch(v.data(), dev, count, 6.0f, P, nullptr), DI_ERANGE, "pairs past 2^29");
    expect(di_interface_work_bytes(v.data(), count), DI_ERANGE, "work bytes past 2^29");
    it = keep, it.l1 = 1 << 15, it.l2 = 1 << 14;
    expect(di_interface_labels_batch(v.data(), dev, count, 6.0f, P, nullptr), DI_ERANGE, "pairs = 2^29");
    it = keep, it.a0 = 1 << 24;
    expect(di_interface_labels_batch(v.data(), dev, count, 6.0f, P, nullptr), DI_ERANGE, "2^24 atoms");
    it = keep, it.a1 = INT32_MAX;
    expect(di_interface_labels_batch(v.data(), dev, count, 6.0f, P, nullptr), DI_ERANGE, "INT32_MAX atoms");
    it = keep;
    expect(di_interface_work_bytes(v.data(), count), nb, "restored");
    expect(di_interface_labels_batch_check(v.data(), dev, count, 6.0f, P), DI_OK, "restored check");
  }
  {  // counts outside 1 .. DI_BATCH_MAX never read the table
    auto v = make(1);
    for (int count : {0, -1, INT32_MIN}) {
      expect(di_interface_work_bytes(v.data(), count), DI_EINVAL, "count < 1");
      expect(di_interface_labels_batch(v.data(), dev, count, 6.0f, P, nullptr), DI_EINVAL, "count < 1");
    }
    for (int count : {DI_BATCH_MAX + 1, INT32_MAX}) {
      expect(di_interface_work_bytes(v.data(), count), DI_ERANGE, "count > DI_BATCH_MAX");
      expect(di_interface_labels_batch(v.data(), dev, count, 6.0f, P, nullptr), DI_ERANGE, "count > DI_BATCH_MAX");
    }
    expect(di_interface_work_bytes(nullptr, 1), DI_EINVAL, "NULL table");
    expect(di_interface_labels_batch(nullptr, dev, 1, 6.0f, P, nullptr), DI_EINVAL, "NULL table");
    expect(di_interface_labels_batch(v.data(), nullptr, 1, 6.0f, P, nullptr), DI_EINVAL, "NULL device table");
    expect(di_interface_labels_batch(v.data(), dev, 1, 6.0f, nullptr, nullptr), DI_EINVAL, "NULL work");
  }
  if (failures) return 1;
  std::puts("host_interface_san: ok");
  return 0;
}
