// CPU check of plan_mx in torchstore_amd/csrc/plan.h.
//
// A plain program: exit status 0 and "mx_plan_check ok" when every check
// holds.  Built by tests/test_native_mx_plan.py with the host compiler and
// -fsanitize=address,undefined.  It includes the planner header and nothing
// else of the extension.

#include "plan.h"

#include <cstdio>
#include <cstdlib>
#include <string>

static int g_failures = 0;

#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      if (++g_failures <= 20) {                                 \
        std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
        std::fprintf(stderr, __VA_ARGS__);                      \
        std::fprintf(stderr, "\n");                             \
      }                                                         \
    }                                                           \
  } while (0)

template <typename F>
static std::string thrown(F&& f) {
  try {
    f();
  } catch (const std::runtime_error& e) {
    return e.what();
  }
  return "";
}

static const uintptr_t kW = 0x1000, kQ = 0x2000, kS = 0x3001;  // scales: bytes

static Plan<MxDesc> one(QuantIn it) { return plan_mx({it}); }

static void check_eligibility_and_rejections() {
  for (int dtype : {0, 1, 2}) {
    const MxDesc d = one({kW, kQ, kS, 3, 256, dtype}).descs[0];
    CHECK(d.fast == 1, "aligned whole blocks are fast");
    CHECK(d.dtype == (uint32_t)dtype && d.cols == 256 && d.nblk == 8 &&
              d.nblocks == 24 && d.rows == 3 && d.wide == kW &&
              d.payload == kQ && d.scales == kS,
          "geometry");
    CHECK(one({kW + 4, kQ, kS, 3, 256, dtype}).descs[0].fast == 0, "wide base");
    CHECK(one({kW, kQ + 1, kS, 3, 256, dtype}).descs[0].fast == 0,
          "payload base");
    CHECK(one({kW, kQ + 8, kS, 3, 256, dtype}).descs[0].fast == 0,
          "payload base at 8 mod 16");
    CHECK(one({kW, kQ, kS, 3, 32, dtype}).descs[0].fast == 1, "one block");
    for (uint64_t cols : {1, 16, 31, 33, 48, 255, 257})
      CHECK(one({kW, kQ, kS, 3, cols, dtype}).descs[0].fast == 0,
            "cols %llu: a short last block is generic",
            (unsigned long long)cols);
    CHECK(one({kW, kQ, kS + 6, 3, 256, dtype}).descs[0].fast == 1,
          "scales need no alignment");
  }
  CHECK(thrown([&] { one({kW, kQ, kS, 1, 32, -1}); }) == "unsupported dtype",
        "-1");
  CHECK(thrown([&] { one({kW, kQ, kS, 0, 32, 3}); }) == "unsupported dtype",
        "dtype is checked before empty tensors are dropped");
  const std::string big = "tensor too large for one mx descriptor";
  CHECK(thrown([&] { one({kW, kQ, kS, 1, (uint64_t)UINT32_MAX + 1, 0}); }) ==
            big, "cols");
  CHECK(thrown([&] { one({kW, kQ, kS, (1ull << 31) + 1, 1, 0}); }) == big,
        "blocks");
  CHECK(thrown([&] { one({kW, kQ, kS, (1ull << 30) + 1, 33, 0}); }) == big,
        "blocks of short rows");
  CHECK(one({kW, kQ, kS, 1ull << 31, 32, 2}).units ==
            (1ull << 31) / kMxUnitBlocks, "2^31 blocks are fine");
  CHECK(one({kW, kQ, kS, 1, UINT32_MAX, 2}).descs[0].nblk == (1u << 27),
        "the longest row");
  CHECK(thrown([&] { one({kW + 2, kQ, kS, 1, 32, 0}); }) == "misaligned tensor",
        "f32 at 2 mod 4");
  CHECK(thrown([&] { one({kW + 1, kQ, kS, 1, 32, 2}); }) == "misaligned tensor",
        "bf16 at an odd address");
  CHECK(one({kW + 2, kQ, kS, 1, 32, 1}).descs.size() == 1,
        "f16 at 2 mod 4 is fine");
}

// Walks the units of descs[i] the way quant_mx_kernel decodes them: every
// one of the 256 block slots of a unit is block local * 256 + slot, live
// when below nblocks.  Fast blocks sit at element 32 b / payload byte 16 b;
// generic ones are placed by row and column.  Every element and every
// payload byte of the tensor must be covered exactly once, every scale once.
static void check_coverage(const Plan<MxDesc>& p, size_t i) {
  const MxDesc& d = p.descs[i];
  const uint64_t end =
      i + 1 < p.descs.size() ? p.descs[i + 1].units_prefix : p.units;
  const uint64_t row_bytes = ((uint64_t)d.cols + 1) / 2;
  std::vector<uint8_t> elem(d.rows * d.cols, 0);
  std::vector<uint8_t> byte(d.rows * row_bytes, 0);
  std::vector<uint8_t> scale(d.nblocks, 0);
  CHECK(end - d.units_prefix == (d.nblocks + kMxUnitBlocks - 1) / kMxUnitBlocks,
        "unit count of tensor %zu", i);
  for (uint64_t local = 0; local < end - d.units_prefix; ++local) {
    CHECK(local * kMxUnitBlocks < d.nblocks, "unit %llu holds no block",
          (unsigned long long)local);
    for (uint32_t slot = 0; slot < kMxUnitBlocks; ++slot) {
      const uint64_t gb = local * kMxUnitBlocks + slot;
      if (gb >= d.nblocks) continue;
      uint64_t eoff, poff;
      uint32_t n;
      if (d.fast) {
        eoff = gb * kMxBlock;
        poff = gb * (kMxBlock / 2);
        n = kMxBlock;
      } else {
        const uint64_t row = gb / d.nblk;
        const uint32_t b = (uint32_t)(gb - row * d.nblk);
        const uint32_t col0 = b * kMxBlock;
        eoff = row * d.cols + col0;
        poff = row * row_bytes + b * (kMxBlock / 2);
        n = d.cols - col0 < kMxBlock ? d.cols - col0 : kMxBlock;
      }
      CHECK(n >= 1 && eoff + n <= elem.size(), "block %llu leaves the tensor",
            (unsigned long long)gb);
      CHECK(poff + (n + 1) / 2 <= byte.size(),
            "block %llu leaves the payload", (unsigned long long)gb);
      if (eoff + n > elem.size() || poff + (n + 1) / 2 > byte.size()) return;
      for (uint32_t c = 0; c < n; ++c) ++elem[eoff + c];
      for (uint32_t j = 0; j < (n + 1) / 2; ++j) ++byte[poff + j];
      ++scale[gb];
    }
  }
  for (size_t k = 0; k < elem.size(); ++k)
    CHECK(elem[k] == 1, "rows %llu cols %u fast %u: element %zu covered %u times",
          (unsigned long long)d.rows, d.cols, d.fast, k, elem[k]);
  for (size_t k = 0; k < byte.size(); ++k)
    CHECK(byte[k] == 1, "rows %llu cols %u fast %u: byte %zu covered %u times",
          (unsigned long long)d.rows, d.cols, d.fast, k, byte[k]);
  for (size_t k = 0; k < scale.size(); ++k)
    CHECK(scale[k] == 1, "scale %zu covered %u times", k, scale[k]);
}

static void check_prefixes_and_coverage() {
  const uint64_t cols[] = {1, 2, 31, 32, 33, 63, 64, 65, 200, 4128};
  const uint64_t rows[] = {1, 7, 256, 257};
  // every case in ONE plan, empty tensors among them
  std::vector<QuantIn> in = {{kW, kQ, kS, 0, 32, 2}, {kW, kQ, kS, 7, 0, 2}};
  for (uint64_t c : cols)
    for (uint64_t r : rows) {
      in.push_back({kW, kQ, kS, r, c, 2});
      in.push_back({kW + 2, kQ, kS, r, c, 1});  // same shapes, generic
    }
  in.push_back({kW, kQ, kS, 0, 0, 0});
  const Plan<MxDesc> p = plan_mx(in);
  CHECK(p.descs.size() == in.size() - 3, "tensors without elements are dropped");
  uint64_t units = 0;
  size_t i = 0;
  for (const QuantIn& it : in) {
    if (it.rows == 0 || it.cols == 0) continue;
    if (i >= p.descs.size()) break;
    const MxDesc& d = p.descs[i];
    const uint64_t nblk = (it.cols + 31) / 32;
    CHECK(d.units_prefix == units, "prefix of tensor %zu", i);
    CHECK(d.cols == it.cols && d.rows == it.rows && d.nblk == nblk &&
              d.nblocks == it.rows * nblk,
          "geometry of tensor %zu", i);
    CHECK(d.fast == ((it.wide & 15) == 0 && it.cols % 32 == 0 ? 1u : 0u),
          "fast flag of tensor %zu", i);
    units += (it.rows * nblk + 255) / 256;
    check_coverage(p, i);
    ++i;
  }
  CHECK(p.units == units, "unit total %llu != %llu",
        (unsigned long long)p.units, (unsigned long long)units);
  CHECK(plan_mx({}).units == 0 && plan_mx({}).descs.empty(), "empty plan");
  CHECK(one({kW, kQ, kS, 1, 256 * 32, 0}).units == 1, "256 blocks are one unit");
  CHECK(one({kW, kQ, kS, 1, 257 * 32, 0}).units == 2, "257 blocks are two");
}

int main() {
  check_eligibility_and_rejections();
  check_prefixes_and_coverage();
  if (g_failures) {
    std::fprintf(stderr, "mx_plan_check: %d check(s) failed\n", g_failures);
    return 1;
  }
  std::puts("mx_plan_check ok");
  return 0;
}
