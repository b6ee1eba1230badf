// CPU check of the launch planners in torchstore_amd/csrc/plan.h.
//
// A plain program: exit status 0 and "plan_check ok" when every check holds.
// Built by tests/test_native_plan.py with the host compiler and
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

static const uintptr_t kSrc = 0x10000000, kDst = 0x20000000;

// ---------------------------------------------------------------------------
// slice plan
// ---------------------------------------------------------------------------

struct Slice {
  uint64_t shape[kMaxDims];
  int64_t sst[kMaxDims], dst[kMaxDims];
  SliceIn in;
};

// `rows` rows of row_bytes under `ndim` outer dims (the rows sit in the
// first dim, the others are 1); row strides 16B-aligned and wider than a row
static void make_slice(Slice& s, uint64_t row_bytes, uint64_t rows,
                       uint32_t ndim) {
  const int64_t stride = (int64_t)((row_bytes + 15) / 16 * 16) * 2;
  for (uint32_t k = 0; k < ndim; ++k) {
    s.shape[k] = k == 0 ? rows : 1;
    s.sst[k] = stride;
    s.dst[k] = stride + 64;
  }
  s.in = SliceIn{kSrc, kDst, row_bytes, s.shape, s.sst, s.dst, ndim};
}

// Walks the units of descs[i] the way copy_slices_kernel decodes them and
// checks that they cover every byte of every row exactly once.  Units come
// in growing order, so within a row each one must start where the last ended.
static void check_coverage(const Plan<SliceDesc>& p, size_t i, uint32_t tile) {
  const SliceDesc& d = p.descs[i];
  const uint64_t end =
      i + 1 < p.descs.size() ? p.descs[i + 1].units_prefix : p.units;
  std::vector<uint64_t> covered(d.rows, 0);
  for (uint64_t local = 0; local < end - d.units_prefix; ++local) {
    if (d.rows_per_unit > 1) {
      const uint64_t row0 = local * d.rows_per_unit;
      CHECK(row0 < d.rows, "packed unit %llu past the rows",
            (unsigned long long)local);
      if (row0 >= d.rows) return;
      const uint64_t nrows =
          d.rows - row0 < d.rows_per_unit ? d.rows - row0 : d.rows_per_unit;
      for (uint64_t r = row0; r < row0 + nrows; ++r) {
        CHECK(covered[r] == 0, "row %llu packed twice", (unsigned long long)r);
        covered[r] += d.row_bytes;
      }
      continue;
    }
    const uint64_t row = local / d.tiles_per_row;
    const uint32_t t = (uint32_t)(local % d.tiles_per_row);
    CHECK(row < d.rows, "unit %llu past the rows", (unsigned long long)local);
    if (row >= d.rows) return;
    const uint32_t start = t * tile;
    CHECK(start <= d.row_bytes, "tile %u starts past the row", t);
    const uint32_t len =
        tile < d.row_bytes - start ? tile : d.row_bytes - start;
    CHECK(covered[row] == start, "row_bytes %u: tile %u starts at %u after %llu",
          d.row_bytes, t, start, (unsigned long long)covered[row]);
    covered[row] += len;
  }
  for (uint64_t r = 0; r < d.rows; ++r) {
    CHECK(covered[r] == d.row_bytes,
          "row_bytes %u rows %llu ndim %u tile %u: row %llu has %llu bytes "
          "covered (rows_per_unit %u, tiles_per_row %u)",
          d.row_bytes, (unsigned long long)d.rows, d.ndim, tile,
          (unsigned long long)r, (unsigned long long)covered[r],
          d.rows_per_unit, d.tiles_per_row);
  }
}

static uint64_t expected_units(const SliceDesc& d, uint32_t tile) {
  if (d.rows_per_unit > 1)
    return (d.rows + d.rows_per_unit - 1) / d.rows_per_unit;
  const uint64_t tiles = ((uint64_t)d.row_bytes + tile - 1) / tile;
  return d.rows * (tiles ? tiles : 1);
}

static void check_slice_plan() {
  std::vector<uint64_t> widths;
  for (uint64_t rb = 16; rb <= 70000; rb += 16) widths.push_back(rb);
  for (uint64_t rb : {0, 1, 2, 17, 100, 4098, 16383, 16385, 32767, 32769,
                      65535, 65537, 69999})
    widths.push_back(rb);
  for (uint32_t tile : {16384u, 32768u}) {
    // every case in ONE plan, so the prefix sums run over mixed descriptors
    std::vector<Slice> slices;
    slices.reserve(widths.size() * 7);
    for (uint64_t rb : widths) {
      for (uint32_t ndim : {0u, 1u, 2u}) {
        for (uint64_t rows : {1, 2, 5}) {
          if (ndim == 0 && rows != 1) continue;  // no outer dim: one row
          slices.emplace_back();
          make_slice(slices.back(), rb, rows, ndim);
        }
      }
    }
    std::vector<SliceIn> in;
    for (Slice& s : slices) {  // the vector no longer moves: fix the pointers
      s.in.shape = s.shape;
      s.in.src_stride = s.sst;
      s.in.dst_stride = s.dst;
      in.push_back(s.in);
    }
    const Plan<SliceDesc> p = plan_slices(in, tile);
    CHECK(p.descs.size() == in.size(), "one descriptor per slice");
    uint64_t units = 0;
    for (size_t i = 0; i < p.descs.size(); ++i) {
      const SliceDesc& d = p.descs[i];
      CHECK(d.units_prefix == units, "prefix of slice %zu", i);
      CHECK(d.rows == slice_rows(in[i]) && d.row_bytes == in[i].row_bytes &&
                d.ndim == in[i].ndim && d.src == kSrc && d.dst == kDst,
            "geometry of slice %zu", i);
      units += expected_units(d, tile);
      check_coverage(p, i, tile);
    }
    CHECK(p.units == units, "unit total %llu != %llu",
          (unsigned long long)p.units, (unsigned long long)units);
  }

  // row-pack eligibility, 5 rows under one outer dim unless said otherwise
  auto rows_per_unit = [](uint64_t rb, uint64_t rows, uint32_t ndim,
                          auto&& tweak) {
    Slice s;
    make_slice(s, rb, rows, ndim);
    tweak(s);
    const Plan<SliceDesc> p = plan_slices({s.in}, 16384);
    const SliceDesc& d = p.descs[0];
    if (d.rows_per_unit > 1) {
      CHECK(d.tiles_per_row == 1, "packed slices have no tiles");
    } else {
      CHECK(d.tiles_per_row == (rb + 16383) / 16384 || (rb == 0),
            "row_bytes %llu keeps its tiles, has %u", (unsigned long long)rb,
            d.tiles_per_row);
    }
    return d.rows_per_unit;
  };
  auto none = [](Slice&) {};
  CHECK(rows_per_unit(16, 5, 1, none) == 4096, "16 B rows");
  CHECK(rows_per_unit(8192, 5, 1, none) == 8, "8 KiB rows");
  CHECK(rows_per_unit(32752, 5, 1, none) == 2, "32752 packs two rows");
  CHECK(rows_per_unit(32768, 5, 1, none) == 2, "32768 packs two rows");
  CHECK(rows_per_unit(32784, 5, 1, none) == 1, "32784: one row is no pack");
  CHECK(rows_per_unit(65520, 5, 1, none) == 1, "65520: one row is no pack");
  CHECK(rows_per_unit(65536, 5, 1, none) == 1, "65536 is not small");
  CHECK(rows_per_unit(8192, 1, 1, none) == 1, "one row");
  CHECK(rows_per_unit(8192, 1, 0, none) == 1, "no outer dim");
  CHECK(rows_per_unit(8192, 5, 2, none) == 1, "two outer dims");
  CHECK(rows_per_unit(8200, 5, 1, none) == 1, "row not a multiple of 16");
  CHECK(rows_per_unit(8192, 5, 1, [](Slice& s) { s.in.src += 8; }) == 1,
        "misaligned source");
  CHECK(rows_per_unit(8192, 5, 1, [](Slice& s) { s.in.dst += 4; }) == 1,
        "misaligned destination");
  CHECK(rows_per_unit(8192, 5, 1, [](Slice& s) { s.sst[0] += 8; }) == 1,
        "misaligned source stride");
  CHECK(rows_per_unit(8192, 5, 1, [](Slice& s) { s.dst[0] += 8; }) == 1,
        "misaligned destination stride");

  Slice s;
  make_slice(s, 64, 1, 0);
  s.in.ndim = kMaxDims + 1;
  CHECK(thrown([&] { plan_slices({s.in}, 16384); }) == "too many dims", "dims");
  make_slice(s, (uint64_t)UINT32_MAX + 1, 1, 0);
  CHECK(thrown([&] { plan_slices({s.in}, 16384); }) == "row too large", "row");
  make_slice(s, UINT32_MAX, 1, 0);
  CHECK(plan_slices({s.in}, 32768).units == (1u << 17), "largest row");
}

// ---------------------------------------------------------------------------
// flat plan
// ---------------------------------------------------------------------------

static SliceIn flat_in(uintptr_t src, uintptr_t dst, uint64_t n) {
  return SliceIn{src, dst, n, nullptr, nullptr, nullptr, 0};
}

static void check_flat_plan() {
  const uint32_t span = 16384;
  Plan<FlatDesc> p;
  const std::vector<SliceIn> good = {
      flat_in(kSrc, kDst, span - 16), flat_in(kSrc + 0x100000, kDst, 0),
      flat_in(kSrc, kDst + 0x100000, span), flat_in(kSrc, kDst, span + 16)};
  CHECK(plan_flat(good, span, p), "aligned ranges are flat");
  CHECK(p.descs.size() == 3, "the zero-byte entry is dropped");
  CHECK(p.units == 4, "1 + 1 + 2 units, got %llu", (unsigned long long)p.units);
  const uint64_t prefix[] = {0, 1, 2};
  const uint64_t nbytes[] = {span - 16, span, span + 16};
  for (size_t i = 0; i < p.descs.size() && i < 3; ++i) {
    CHECK(p.descs[i].units_prefix == prefix[i], "flat prefix %zu", i);
    CHECK(p.descs[i].nbytes == nbytes[i], "flat nbytes %zu", i);
  }
  CHECK(p.descs[1].src == kSrc && p.descs[1].dst == kDst + 0x100000, "ptrs");

  CHECK(plan_flat({flat_in(kSrc, kDst, 0), flat_in(kSrc, kDst, 0)}, span, p),
        "empty copies are flat");
  CHECK(p.descs.empty() && p.units == 0, "and yield no units");

  // each reason on its own, after entries that qualify
  uint64_t two = 2;
  int64_t st = 64;
  const SliceIn odd[] = {
      flat_in(kSrc + 2, kDst, 4096),                 // source alignment
      flat_in(kSrc, kDst + 8, 4096),                 // destination alignment
      flat_in(kSrc, kDst, 4098),                     // length
      flat_in(kSrc + 1, kDst, 0),                    // even when empty
      flat_in(kSrc, kDst, (uint64_t)UINT32_MAX + 1), // 4 GiB and more
      SliceIn{kSrc, kDst, 64, &two, &st, &st, 1},    // has rows
  };
  for (const SliceIn& o : odd) {
    std::vector<SliceIn> in = good;
    in.push_back(o);
    CHECK(!plan_flat(in, span, p), "odd entry %d keeps the launch general",
          (int)(&o - odd));
  }
}

// ---------------------------------------------------------------------------
// quant plan
// ---------------------------------------------------------------------------

static void check_quant_plan() {
  const uintptr_t w = 0x1000, q = 0x2000, s = 0x3000;
  auto one = [](QuantIn it) { return plan_quant({it}); };
  for (int dtype : {0, 1, 2}) {
    CHECK(one({w, q, s, 3, 256, dtype}).descs[0].fast == 1, "aligned is fast");
    CHECK(one({w, q, s, 3, 256, dtype}).descs[0].dtype == (uint32_t)dtype, "dt");
    CHECK(one({w + 4, q, s, 3, 256, dtype}).descs[0].fast == 0, "wide base");
    CHECK(one({w, q + 1, s, 3, 256, dtype}).descs[0].fast == 0, "payload base");
    CHECK(one({w, q, s, 3, 264, dtype}).descs[0].fast == 0, "cols not a multiple of 16");
    CHECK(one({w, q, s + 4, 3, 144, dtype}).descs[0].fast == 1,
          "scales need 4B only; a short last block stays fast");
  }
  CHECK(thrown([&] { one({w, q, s, 1, 128, -1}); }) == "unsupported dtype", "-1");
  CHECK(thrown([&] { one({w, q, s, 0, 128, 3}); }) == "unsupported dtype",
        "dtype is checked before empty tensors are dropped");
  const std::string big = "tensor too large for one quant descriptor";
  CHECK(thrown([&] { one({w, q, s, 1, (uint64_t)UINT32_MAX + 1, 0}); }) == big,
        "cols");
  CHECK(thrown([&] { one({w, q, s, (1ull << 31) + 1, 1, 0}); }) == big, "blocks");
  CHECK(one({w, q, s, 1ull << 31, 128, 2}).units == (1ull << 31) / 64, "2^31 ok");
  CHECK(thrown([&] { one({w, q, s + 2, 1, 128, 0}); }) ==
            "scales must be 4B aligned", "scales");
  CHECK(thrown([&] { one({w + 2, q, s, 1, 128, 0}); }) == "misaligned tensor",
        "f32 at 2 mod 4");
  CHECK(thrown([&] { one({w + 1, q, s, 1, 128, 2}); }) == "misaligned tensor",
        "bf16 at an odd address");
  CHECK(one({w + 2, q, s, 1, 128, 1}).descs.size() == 1, "f16 at 2 mod 4 is fine");

  const uint64_t cols[] = {1, 127, 128, 129, 144};
  const uint32_t nblk[] = {1, 1, 1, 2, 2};
  std::vector<QuantIn> in = {{w, q, s, 0, 128, 2}, {w, q, s, 7, 0, 2}};
  for (uint64_t c : cols) in.push_back({w, q, s, 100, c, 2});
  in.push_back({w, q, s, 64, 128, 0});
  in.push_back({w, q, s, 65, 128, 0});
  const Plan<QuantDesc> p = plan_quant(in);
  CHECK(p.descs.size() == 7, "tensors without elements are dropped");
  if (p.descs.size() != 7) return;
  uint64_t units = 0;
  for (size_t i = 0; i < 5 && i < p.descs.size(); ++i) {
    const QuantDesc& d = p.descs[i];
    CHECK(d.cols == cols[i] && d.nblk == nblk[i] && d.nblocks == 100 * nblk[i],
          "cols %llu: nblk %u nblocks %u", (unsigned long long)cols[i], d.nblk,
          d.nblocks);
    CHECK(d.units_prefix == units, "quant prefix %zu", i);
    units += nblk[i] == 1 ? 2 : 4;  // ceil(100 / 64), ceil(200 / 64)
  }
  CHECK(p.descs[5].units_prefix == units, "prefix after the short-row ones");
  CHECK(p.descs[6].units_prefix == units + 1, "64 blocks are one unit");
  CHECK(p.units == units + 1 + 2, "65 blocks are two");
}

int main() {
  check_slice_plan();
  check_flat_plan();
  check_quant_plan();
  if (g_failures) {
    std::fprintf(stderr, "plan_check: %d check(s) failed\n", g_failures);
    return 1;
  }
  std::puts("plan_check ok");
  return 0;
}
