// Stand-alone driver for the host side of csrc/contact_examples.hip under AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/test_examples_host_sanitized.py builds both with
// -Xarch_host -fsanitize=address,undefined and runs this program; device code is not sanitized and
// nothing is launched: every call here is refused, or is a *_check form, before any launch).
// It walks the validation and the size / offset arithmetic of di_examples_labels_work_bytes,
// di_examples_labels_batch(_check) and di_examples_gather_batch(_check) with tables of every size up to
// DI_BATCH_MAX + 1, extreme shapes and dummy pointers that are never dereferenced.
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

int main() {
  void* const P = reinterpret_cast<void*>(16 * 1024);  // 16-B aligned, never dereferenced
  const int32_t shapes[][2] = {{1, 1}, {3, 5}, {145, 145}, {7, 400}, {300, 300}, {4096, 4096}, {1, 1 << 28}};
  const int nshapes = sizeof(shapes) / sizeof(shapes[0]);

  auto label_items = [&](int count) {
    std::vector<di_examples_item> v(count);   // exactly count items: a read past the table is a heap overflow
    for (int i = 0; i < count; ++i) {
      di_examples_item it = {};
      it.examples = P, it.labels = reinterpret_cast<uint8_t*>(P);
      it.l1 = shapes[i % nshapes][0], it.l2 = shapes[i % nshapes][1];
      it.n = (int64_t)it.l1 * it.l2;
      v[i] = it;
    }
    return v;
  };
  auto gather_items = [&](int count) {
    std::vector<di_examples_item> v(count);
    for (int i = 0; i < count; ++i) {
      di_examples_item it = {};
      it.examples = it.logits = it.pool_logits = P, it.pool_labels = reinterpret_cast<uint8_t*>(P);
      it.l1 = shapes[i % nshapes][0], it.l2 = shapes[i % nshapes][1];
      it.n = 1 + i, it.out_off = 7 * i, it.total = 8 * i + 1;
      v[i] = it;
    }
    return v;
  };
  auto* dev = reinterpret_cast<const di_examples_item*>(P);

  for (int count : {1, 2, 7, 1023, DI_BATCH_MAX}) {
    auto v = label_items(count);
    const int64_t nb = di_examples_labels_work_bytes(v.data(), count);
    expect(nb > 0 && nb % 16 == 0, 1, "labels work bytes");
    int64_t at = ((int64_t)count * 4 + 15) / 16 * 16;
    for (int i = 0; i < count; ++i) {
      expect(v[i].work_off, at, "labels work_off");
      at += ((v[i].n + 31) / 32 * 4 + 15) / 16 * 16;
    }
    expect(nb, at, "labels total");
    expect(di_examples_labels_batch_check(DI_I64, v.data(), dev, count, P), DI_OK, "labels check");
    expect(di_examples_labels_batch_check(DI_I32, v.data(), dev, count, P), DI_OK, "labels check int32");
    v[count - 1].work_off += 16;
    expect(di_examples_labels_batch(DI_I64, v.data(), dev, count, P, nullptr), DI_EINVAL, "stale work_off");
    v[count - 1].work_off -= 16;
    v[count / 2].n -= 1;
    expect(di_examples_labels_batch(DI_I64, v.data(), dev, count, P, nullptr), DI_EINVAL, "n != l1 * l2");
    v[count / 2].n += 1;
    v[count / 2].l1 = INT32_MAX, v[count / 2].l2 = INT32_MAX, v[count / 2].n = (int64_t)INT32_MAX * INT32_MAX;
    expect(di_examples_labels_batch(DI_I64, v.data(), dev, count, P, nullptr), DI_ERANGE, "pairs past 2^29");
    expect(di_examples_labels_work_bytes(v.data(), count), DI_ERANGE, "work bytes past 2^29");
    v[count / 2].n = INT64_MAX;
    expect(di_examples_labels_batch(DI_I64, v.data(), dev, count, P, nullptr), DI_EINVAL, "n = INT64_MAX");
    v[count / 2].l1 = INT32_MIN;
    expect(di_examples_labels_batch(DI_I64, v.data(), dev, count, P, nullptr), DI_EINVAL, "l1 = INT32_MIN");

    auto g = gather_items(count);
    for (int dt : {DI_F32, DI_BF16})
      for (int idt : {DI_I64, DI_I32})
        expect(di_examples_gather_batch_check(dt, idt, g.data(), dev, count, reinterpret_cast<int32_t*>(P)), DI_OK,
               "gather check");
    di_examples_item& it = g[count - 1];
    const di_examples_item keep = it;
    it.out_off = INT64_MAX, it.total = INT64_MAX;
    expect(di_examples_gather_batch(DI_F32, DI_I64, g.data(), dev, count, reinterpret_cast<int32_t*>(P), nullptr),
           DI_EINVAL, "out_off = total = INT64_MAX");
    it = keep, it.out_off = INT64_MIN;
    expect(di_examples_gather_batch(DI_F32, DI_I64, g.data(), dev, count, reinterpret_cast<int32_t*>(P), nullptr),
           DI_EINVAL, "out_off = INT64_MIN");
    it = keep, it.n = INT64_MAX;
    expect(di_examples_gather_batch(DI_F32, DI_I64, g.data(), dev, count, reinterpret_cast<int32_t*>(P), nullptr),
           DI_EINVAL, "n = INT64_MAX");
    it = keep, it.n = INT64_MAX, it.total = INT64_MAX, it.out_off = 0;
    expect(di_examples_gather_batch(DI_F32, DI_I64, g.data(), dev, count, reinterpret_cast<int32_t*>(P), nullptr),
           DI_ERANGE, "total past 2^31");
    it = keep, it.l1 = INT32_MAX, it.l2 = INT32_MAX;
    expect(di_examples_gather_batch(DI_BF16, DI_I32, g.data(), dev, count, reinterpret_cast<int32_t*>(P), nullptr),
           DI_ERANGE, "pairs past 2^29");
    for (int bad : {-1, 2, 5, INT32_MAX, INT32_MIN}) {
      it = keep;
      expect(di_examples_gather_batch(bad, DI_I64, g.data(), dev, count, reinterpret_cast<int32_t*>(P), nullptr),
             DI_EINVAL, "bad dtype");
      expect(di_examples_gather_batch(DI_F32, bad, g.data(), dev, count, reinterpret_cast<int32_t*>(P), nullptr),
             DI_EINVAL, "bad index width");
      expect(di_examples_labels_batch(bad, v.data(), dev, count, P, nullptr), DI_EINVAL, "bad index width (labels)");
    }
  }
  {  // counts outside 1 .. DI_BATCH_MAX never read the table
    auto v = label_items(1);
    for (int count : {0, -1, INT32_MIN}) {
      expect(di_examples_labels_work_bytes(v.data(), count), DI_EINVAL, "count < 1");
      expect(di_examples_labels_batch(DI_I64, v.data(), dev, count, P, nullptr), DI_EINVAL, "count < 1");
      expect(di_examples_gather_batch(DI_F32, DI_I64, v.data(), dev, count, reinterpret_cast<int32_t*>(P), nullptr),
             DI_EINVAL, "count < 1");
    }
    for (int count : {DI_BATCH_MAX + 1, INT32_MAX}) {
      expect(di_examples_labels_work_bytes(v.data(), count), DI_ERANGE, "count > DI_BATCH_MAX");
      expect(di_examples_labels_batch(DI_I64, v.data(), dev, count, P, nullptr), DI_ERANGE, "count > DI_BATCH_MAX");
      expect(di_examples_gather_batch(DI_F32, DI_I64, v.data(), dev, count, reinterpret_cast<int32_t*>(P), nullptr),
             DI_ERANGE, "count > DI_BATCH_MAX");
    }
    expect(di_examples_labels_work_bytes(nullptr, 1), DI_EINVAL, "NULL table");
    expect(di_examples_labels_batch(DI_I64, nullptr, dev, 1, P, nullptr), DI_EINVAL, "NULL table");
    expect(di_examples_labels_batch(DI_I64, v.data(), nullptr, 1, P, nullptr), DI_EINVAL, "NULL device table");
    expect(di_examples_labels_batch(DI_I64, v.data(), dev, 1, nullptr, nullptr), DI_EINVAL, "NULL work");
    expect(di_examples_gather_batch(DI_F32, DI_I64, v.data(), dev, 1, nullptr, nullptr), DI_EINVAL, "NULL flags");
  }
  if (failures) return 1;
  std::puts("host_examples_san: ok");
  return 0;
}
