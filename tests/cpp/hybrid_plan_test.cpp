// hybrid_plan_test.cpp -- csrc/hybrid_plan.h (the MSD hybrid's host
// arithmetic): the bucket classes at pinned sizes and their invariants over a
// sweep, the workspace layout against the size expression spelled out, the
// buffer parity and gate predicates, and the piece table against a brute-force
// concatenation of the pieces by segment.  Run under ASan/UBSan by
// tests/test_distrib_plan_cpu.py.
#include <stdio.h>

#include <random>
#include <vector>

#include "hybrid_plan.h"

using namespace lsort::hplan;

static int fails = 0;
#define CHECK(c, ...)                       \
  do {                                      \
    if (!(c)) {                             \
      if (fails++ < 20) {                   \
        fprintf(stderr, "FAIL %s: ", #c);   \
        fprintf(stderr, __VA_ARGS__);       \
        fprintf(stderr, "\n");              \
      }                                     \
    }                                       \
  } while (0)

static BucketPlan plan32(size_t n, double fill = 1.0, bool counting = true) {
  return bucket_plan(n, 65536, fill, 4, counting, 512, 512);
}

static void test_classes() {
  const struct {
    size_t n;
    int cls;
  } pinned[] = {{1ull << 27, 0},
                {1ull << 28, 2},
                {(1ull << 28) + (1ull << 24), 3},
                {1ull << 29, 4},
                {(1ull << 29) + (1ull << 23), 4},
                {1ull << 30, 5},
                {(1ull << 30) + (1ull << 24), 5}};
  for (const auto& c : pinned) {
    const BucketPlan p = plan32(c.n);
    CHECK(p.served && p.cls == c.cls, "n %zu class %d (want %d)", c.n, p.cls, c.cls);
    CHECK(p.block == kBucketClass[c.cls].block, "n %zu block %d", c.n, p.block);
  }
  CHECK(plan32(1ull << 28).need == 4320.0 && plan32(1ull << 28).cap1 == 4352, "2^28: need 4320 <= 4352");
  {
    const BucketPlan p = plan32((1ull << 29) + (1ull << 23));
    CHECK(p.need > 8638.0 && p.need < 8640.0 && p.cap1 == 8704, "2^29 + 2^23: need %f", p.need);
  }
  CHECK(plan32(1ull << 30).cap1 == 17408 && plan32((1ull << 30) + (1ull << 24)).cap1 == 17408, "class 5 cap1");
  CHECK(plan32(1ull << 30).cap == 1024 * 23 && plan32(1ull << 29).cap == 512 * 23, "classes 4, 5 cap");
  CHECK(plan32(1ull << 28).cap == 256 * 23 && plan32(1ull << 28).retry_items == 12, "class 2 second size, retry");
  CHECK(!plan32(1ull << 30, 1.0, false).served, "2^30 without the counting placement");
  CHECK(plan32(1ull << 29, 1.0, false).served, "2^29 without the counting placement");
  // 64-bit keys: rows 0-3 only, the slots in 512-thread blocks
  for (size_t n = 1024; n <= (1ull << 31); n *= 2) {
    const BucketPlan p = bucket_plan(n, 65536, 1.0, 8, false, 512, 512);
    CHECK(p.served && p.cls <= 3 && p.block == 512, "64-bit n %zu class %d", n, p.cls);
    if (p.cls == 3) CHECK(p.cap1 == 5120 && p.cap == 512 * 13, "64-bit class 3 cap1 %u cap %u", p.cap1, p.cap);
  }
  CHECK(bucket_plan(1ull << 20, 65536, 1.0, 8, false, 512, 512).cap1 == 2560, "64-bit class 0 cap1");
  CHECK(bucket_plan(1ull << 28, 65536, 1.0, 8, false, 256, 512).cap1 == 4352, "64-bit, 256-thread blocks");
  // range fill
  {
    const size_t n = 1ull << 27;
    const uint64_t span = (uint64_t)(0.8 * (double)(1ull << 27));
    const double fill = range_fill(span, 27);
    CHECK(fill == (double)span / (double)(1ull << 27), "range fill %f", fill);
    CHECK(plan32(n, fill).mean == (double)n / (65536 * fill), "range mean");
    CHECK(std::fabs(plan32(n, fill).mean - (double)n / (65536 * 0.8)) < 1e-3, "range mean ~ n / (NB 0.8)");
    CHECK(range_fill(0, 32) == 1.0, "no span");
  }
  // invariants over a sweep
  for (double fill : {0.55, 0.8, 1.0}) {
    std::vector<size_t> ns;
    for (int lg = 10; lg <= 30; ++lg)
      for (long d : {-7L, -1L, 0L, 1L, 5L, 1001L}) {
        if (lg == 10 && d < 0) continue;
        ns.push_back((size_t)((long)(1ull << lg) + d));
      }
    for (int lg = 20; lg <= 29; ++lg) ns.push_back((1ull << lg) + (1ull << (lg - 1)) + 3);
    for (int lg = 23; lg <= 24; ++lg) {
      ns.push_back((1ull << 29) + (1ull << lg));
      ns.push_back((1ull << 30) + (1ull << lg));
      ns.push_back((1ull << 28) + (1ull << lg) - 3);
    }
    std::sort(ns.begin(), ns.end());
    int prev = 0, served_n = 0;
    bool prev_served = true;
    for (size_t n : ns) {
      if (n > (1ull << 30) + (1ull << 24)) continue;
      const BucketPlan p = plan32(n, fill);
      CHECK(p.cls >= prev, "fill %.2f n %zu: class %d after %d", fill, n, p.cls, prev);
      CHECK(prev_served || !p.served, "fill %.2f n %zu: served after a larger n was not", fill, n);
      prev = p.cls;
      prev_served = p.served;
      if (!p.served) continue;
      ++served_n;
      CHECK((double)p.cap1 >= p.need, "fill %.2f n %zu: cap1 %u < need %f", fill, n, p.cap1, p.need);
      CHECK(p.cap > p.cap1, "fill %.2f n %zu: cap %u cap1 %u", fill, n, p.cap, p.cap1);
      CHECK(p.cap < 65536, "fill %.2f n %zu: cap %u (16-bit cell starts)", fill, n, p.cap);
      CHECK(p.cap1 == (uint32_t)(p.block * class_items1(p.cls, 256)) && p.block == class_block(p.cls, 256),
            "plan and dispatch from one table");
    }
    CHECK(served_n > 100, "sweep too small: %d", served_n);
    CHECK(fill < 1.0 || prev_served, "uniform keys are served up to 2^30 + 2^24");
  }
}

static void test_layout() {
  const struct {
    int bits;
    uint32_t nseg0;
    int depths;
  } shapes[] = {{4, 1, 4}, {8, 1, 2}, {4, 5, 3}, {8, 16, 1}};
  for (const auto& s : shapes)
    for (bool rsv : {false, true}) {
      const size_t n = (1u << 22) + 5;
      const uint32_t radix = 1u << s.bits, tile = s.bits == 4 ? 4096 : 8192;
      const uint32_t NB = s.nseg0 << (s.bits * s.depths), rnc = s.nseg0 * radix, rns = rnc * kRsvRanges;
      const uint32_t T0 = (uint32_t)((n + tile - 1) / tile) + s.nseg0 - 1, Tt = T0;
      const size_t rbound = rsv_capacity_bound_nc(n, rnc, kRsvBlocks * 256 * 4, tile);
      CHECK(rbound >= n + (size_t)rns * tile, "slices hold n keys and a partial tile each");
      const uint32_t tb1 = (uint32_t)((rbound + tile - 1) / tile) + rns;
      uint32_t TB = 0;
      for (int k = 0; k < s.depths; ++k)
        TB = std::max(TB, tile_bound(k, T0, Tt, tb1, rsv, s.nseg0 << (s.bits * k)));
      CHECK(tile_bound(0, T0, Tt, tb1, rsv, s.nseg0) == T0, "depth 0's rows");
      if (s.depths > 1)
        CHECK(tile_bound(1, T0, Tt, tb1, rsv, rnc) == (rsv ? tb1 : Tt + rnc), "depth 1's rows");
      const HybLayout L = hyb_layout(TB, NB, rnc);
      // the regions in order with their sizes
      const size_t off[] = {L.tiles[0], L.tiles[1], L.segbase, L.cstart[0], L.cstart[1], L.nsize,  L.ctile0[0],
                            L.ctile0[1], L.ntl,     L.ctr,     L.olist,     L.flist,     L.flist2, L.rpart,
                            L.rslice,    L.words};
      const size_t size[] = {(size_t)TB * 4,
                             (size_t)TB * 4,
                             NB,
                             NB,
                             NB,
                             NB,
                             (size_t)NB + 1,
                             (size_t)NB + 1,
                             NB,
                             16,
                             1024,
                             NB,
                             NB,
                             (size_t)8 * 32 * rnc,
                             3 * (size_t)rns + 16};
      CHECK(off[0] == 0, "the block starts with the tiles");
      for (int i = 0; i < 15; ++i)
        CHECK(off[i] + size[i] == off[i + 1], "bits %d nseg %u region %d: %zu + %zu != %zu", s.bits, s.nseg0, i, off[i],
              size[i], off[i + 1]);
      CHECK(L.tiles[0] % 4 == 0 && L.tiles[1] % 4 == 0, "tile tables 16-byte aligned");
      // the size as the driver computed it before the layout struct
      const size_t w_tiles = (size_t)TB * 4;
      const size_t rsv_words = (size_t)8 * 32 * rnc + 3 * (size_t)rns + 16;
      const size_t words =
          2 * w_tiles + NB + 2 * (size_t)NB + NB + 2 * ((size_t)NB + 1) + NB + 16 + 1024 + NB + NB + rsv_words;
      CHECK(L.words == words, "bits %d nseg %u: words %zu, want %zu", s.bits, s.nseg0, L.words, words);
    }
  // counters and mirror words
  CHECK(kCtrWords == 16 && kCtrOvfN == 15 && kCtrLsdN2 == 7 && kCtrStats == 11, "ctr words");
  CHECK(kHostMaxBucket == 256 && kHostPlanOver1 == 257 && kHostRsvOver == 259 && kHostMaxChild == 260 &&
            kHybSeqWord2 == 510 && kHybSeqWord == 511 && kHostWords == 512,
        "hyb_host words");
}

static void test_predicates() {
  for (int depths = 1; depths <= 4; ++depths)
    for (bool rsv : {false, true}) {
      CHECK(key_buf(0, depths, rsv) == Buf::In && val_buf(0, depths) == Buf::In, "depth 0 reads in");
      CHECK(key_buf(depths, depths, false) == Buf::Out && val_buf(depths, depths) == Buf::Out, "the last writes out");
      for (int k = 1; k <= depths; ++k) {
        if (k == 1 && rsv) {
          CHECK(key_buf(k, depths, rsv) == Buf::Rsv, "reserved depth 0 writes the slices");
          continue;
        }
        CHECK(key_buf(k, depths, rsv) != key_buf(k - 1, depths, rsv), "a pass never writes its source");
        CHECK(key_buf(k, depths, rsv) == val_buf(k, depths), "values travel with the keys");
      }
      if (depths >= 2 && rsv) {
        // the u16 array is neither the last pass's source nor out
        const Buf b = pack16_buf(depths);
        CHECK(b != key_buf(depths - 1, depths, true) && b != Buf::Out && b != Buf::In, "pack16 buffer, %d depths", depths);
      }
    }
  CHECK(pack16_eligible(false, 32, 16, true, 1), "pack16: the full-width keys-only sort");
  CHECK(!pack16_eligible(true, 32, 16, true, 1) && !pack16_eligible(false, 27, 11, true, 1) &&
            !pack16_eligible(false, 32, 16, false, 1) && !pack16_eligible(false, 32, 16, true, 2) &&
            !pack16_eligible(false, 32, 16, true, 0),
        "pack16: not for pieces, ranges, LSD-step buckets, short or no slices");
  const size_t lo = 1ull << 27, hi = (1ull << 30) + (1ull << 24);
  CHECK(!hybrid_serves(0, lo, lo, hi) && hybrid_serves(1, lo, lo, hi) && !hybrid_serves(1, lo - 1, lo, hi) &&
            hybrid_serves(1, hi, lo, hi) && !hybrid_serves(1, hi + 1, lo, hi) && hybrid_serves(2, 1024, lo, hi) &&
            !hybrid_serves(2, 1023, lo, hi) && !hybrid_serves(2, hi + 1, lo, hi),
        "hybrid_serves");
  // uniform 2^28 keys, 16 top digits: the share 2^24 passes, 1.3 shares do not
  CHECK(!top_digit_skewed(1u << 24, 1ull << 28, 16, 1.0, 65536, 5888), "uniform top digit");
  CHECK(top_digit_skewed((1u << 24) + (1u << 24) / 3, 1ull << 28, 16, 1.0, 65536, 5888), "heavy top digit");
  CHECK(top_digit_skewed(4096u * 5400, 1ull << 30, 16, 1.0, 65536, 5888), "buckets over 0.9 of a block");
  CHECK(!piece_child_skewed(4096u * 5000, 12, 5888) && piece_child_skewed(4096u * 5400, 12, 5888), "piece child");
}

static void test_pieces() {
  std::mt19937_64 g(7);
  int cases = 0;
  for (int it = 0; it < 3000; ++it) {
    const size_t np = g() % 65;
    const uint32_t nseg = 1 + (uint32_t)(g() % 16);
    const uint32_t tile = (g() & 1) ? 64 : 17;
    const bool planar = (g() % 4) == 0;
    const uint32_t hi0 = planar ? (uint32_t)(g() % (257 - nseg)) : 0;
    std::vector<uint64_t> off(np), len(np);
    std::vector<uint32_t> seg(np);
    // segments non-decreasing (some unused), about a third of the pieces empty
    uint32_t s = 0;
    for (size_t p = 0; p < np; ++p) {
      if (g() % 3 == 0) s = std::min<uint32_t>(nseg - 1, s + (uint32_t)(g() % 3));
      seg[p] = s;
      len[p] = g() % 3 == 0 ? 0 : 1 + g() % 200;
    }
    // the pieces lie in `in` in a shuffled order with gaps
    std::vector<size_t> order(np);
    for (size_t p = 0; p < np; ++p) order[p] = p;
    std::shuffle(order.begin(), order.end(), g);
    uint64_t pos = 0, n = 0;
    for (size_t p : order) {
      pos += g() % 5;
      off[p] = pos;
      pos += len[p];
      n += len[p];
    }
    std::vector<uint32_t> in(pos + 1);
    for (size_t i = 0; i < in.size(); ++i) in[i] = (uint32_t)g();
    // brute force: the pieces concatenated by segment (table order within one)
    std::vector<uint32_t> want;
    std::vector<uint64_t> seg_start;  // of the populated segments
    std::vector<uint32_t> seg_tile, seg_id;
    uint32_t tiles = 0;
    for (uint32_t sg = 0; sg < nseg; ++sg) {
      bool any = false;
      for (size_t p = 0; p < np; ++p)
        if (seg[p] == sg && len[p]) {
          if (!any) {
            seg_start.push_back(want.size());
            seg_tile.push_back(tiles);
            seg_id.push_back(sg);
          }
          any = true;
          want.insert(want.end(), in.begin() + off[p], in.begin() + off[p] + len[p]);
          tiles += (uint32_t)((len[p] + tile - 1) / tile);
        }
    }
    std::vector<uint64_t> buf;
    const PieceTable t = piece_table(off.data(), len.data(), seg.data(), np, nseg, (size_t)n, 24, 4, n >= 1024, tile,
                                     planar, hi0, [&](size_t words) {
                                       buf.assign(words, 0xAAAAAAAAAAAAAAAAull);
                                       return buf.data();
                                     });
    CHECK(t.ok, "case %d rejected", it);
    if (!t.ok) continue;
    ++cases;
    const uint32_t* h32 = reinterpret_cast<const uint32_t*>(buf.data());
    const uint64_t* hg = buf.data() + t.g64;
    CHECK(t.nseg == seg_start.size() && t.tiles == tiles, "case %d: nseg %u tiles %u", it, t.nseg, t.tiles);
    CHECK(t.words == buf.size() && t.seghi64 + (planar ? (t.nseg + 1) / 2 : 0) == t.words, "case %d: words", it);
    CHECK(2 * t.g64 >= t.cum + t.K + 1 && 2 * t.g64 <= t.cum + t.K + 2, "case %d: gather table 8-byte aligned", it);
    CHECK(t.depths == (n >= 1024 ? 1 : 0), "case %d: depths %d", it, t.depths);
    if (t.nseg != seg_start.size()) continue;
    for (uint32_t cs = 0; cs < t.nseg; ++cs) {
      CHECK(h32[t.cstart + cs] == seg_start[cs], "case %d: cstart[%u]", it, cs);
      CHECK(h32[t.ctile0 + cs] == seg_tile[cs], "case %d: ctile0[%u]", it, cs);
    }
    CHECK(h32[t.ctile0 + t.nseg] == tiles, "case %d: ctile0[nseg]", it);
    // the kept pieces in table order: first tiles, cum, and the gather
    std::vector<uint32_t> got(want.size(), 0);
    uint32_t i = 0, tl = 0, run = 0;
    uint64_t maxlen = 0;
    for (size_t p = 0; p < np; ++p) {
      if (!len[p]) continue;
      CHECK(i < t.K, "case %d: K %u", it, t.K);
      if (i >= t.K) break;
      const uint32_t* pc = h32 + 4 * (size_t)i;
      CHECK(pc[0] == off[p] && pc[1] == len[p] && seg_id[pc[2]] == seg[p] && pc[3] == tl, "case %d: piece %u", it, i);
      CHECK(h32[t.cum + i] == run, "case %d: cum[%u]", it, i);
      CHECK(hg[i] == off[p] && hg[2 * (size_t)t.K + i] == len[p], "case %d: gather piece %u", it, i);
      const uint64_t dst = hg[t.K + i];
      CHECK(dst + len[p] <= got.size(), "case %d: gather destination", it);
      if (dst + len[p] <= got.size())
        for (uint64_t j = 0; j < len[p]; ++j) got[dst + j] = in[off[p] + j];
      if (planar) {
        CHECK(hg[3 * (size_t)t.K + i] == (uint64_t)(hi0 + seg[p]) << 24, "case %d: top byte column", it);
        CHECK(reinterpret_cast<const uint32_t*>(buf.data() + t.seghi64)[pc[2]] == (hi0 + seg[p]) << 24,
              "case %d: seghi", it);
      }
      tl += (uint32_t)((len[p] + tile - 1) / tile);
      run += (uint32_t)len[p];
      maxlen = std::max(maxlen, len[p]);
      ++i;
    }
    CHECK(i == t.K && h32[t.cum + t.K] == n && t.maxlen == maxlen, "case %d: K, cum[K], maxlen", it);
    CHECK(got == want, "case %d: gathered order", it);
    if (t.K) CHECK(t.first_seg == seg_id.front() && t.last_seg == seg_id.back(), "case %d: first / last segment", it);
  }
  CHECK(cases == 3000, "%d cases", cases);
  // digit passes: the fewest that bring the largest segment's mean bucket to <= 8320
  {
    const uint64_t off[] = {0, 1u << 23}, len[] = {1u << 23, 1u << 20};
    const uint32_t seg[] = {0, 3};
    auto none = [](size_t) -> uint64_t* { return nullptr; };
    const size_t n = (1u << 23) + (1u << 20);
    PieceTable t = piece_table(off, len, seg, 2, 5, n, 24, 4, true, 4096, false, 0, none);
    CHECK(t.ok && t.depths == 3 && t.nseg == 2 && t.fill == 1.0, "4-bit depths %d", t.depths);  // 2^23 / 16^3 = 2048
    t = piece_table(off, len, seg, 2, 5, n, 24, 8, true, 8192, false, 0, none);
    CHECK(t.ok && t.depths == 2, "8-bit depths %d", t.depths);
    t = piece_table(off, len, seg, 2, 5, n, 8, 4, true, 4096, false, 0, none);
    CHECK(t.ok && t.depths == 2, "depths within bits: %d", t.depths);
    t = piece_table(off, len, seg, 2, 5, n, 24, 4, false, 4096, false, 0, none);
    CHECK(t.ok && t.depths == 0, "not the hybrid's: %d", t.depths);
    t = piece_table(off, len, seg, 2, 5, n, 0, 4, true, 4096, false, 0, none);
    CHECK(t.ok && t.depths == 0, "no bits to sort: %d", t.depths);
  }
  // rejected tables (tests/test_gpu_pieces.py::test_bad_tables_fail_loudly and the other checks)
  {
    auto none = [](size_t) -> uint64_t* { return nullptr; };
    const uint64_t off2[] = {0, 50}, len2[] = {50, 50};
    const uint32_t bad_order[] = {1, 0}, good[] = {0, 1};
    CHECK(!piece_table(off2, len2, bad_order, 2, 2, 100, 24, 4, true, 4096, false, 0, none).ok, "segments out of order");
    CHECK(piece_table(off2, len2, good, 2, 2, 100, 24, 4, true, 4096, false, 0, none).ok, "a good table");
    const uint64_t off1[] = {0}, len1[] = {100};
    const uint32_t seg_big[] = {2};
    CHECK(!piece_table(off1, len1, seg_big, 1, 2, 100, 24, 4, true, 4096, false, 0, none).ok, "segment >= nseg");
    CHECK(!piece_table(off2, len2, good, 2, 2, 101, 24, 4, true, 4096, false, 0, none).ok, "lengths do not sum to n");
    const uint64_t off_far[] = {0xffffffffull - 10}, len_far[] = {100};
    const uint32_t seg0[] = {0};
    CHECK(!piece_table(off_far, len_far, seg0, 1, 1, 100, 24, 4, true, 4096, false, 0, none).ok, "offset beyond 2^32");
    std::vector<uint64_t> offm(65536), lenm(65536, 1);
    std::vector<uint32_t> segm(65536, 0);
    for (size_t p = 0; p < offm.size(); ++p) offm[p] = p;
    CHECK(!piece_table(offm.data(), lenm.data(), segm.data(), offm.size(), 1, offm.size(), 24, 4, true, 4096, false, 0,
                       none)
               .ok,
          "more than 65535 pieces");
  }
}

int main() {
  test_classes();
  test_layout();
  test_predicates();
  test_pieces();
  if (fails) {
    fprintf(stderr, "%d failures\n", fails);
    return 1;
  }
  printf("OK bucket classes, layout, predicates, piece tables\n");
  return 0;
}
