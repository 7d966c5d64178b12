// hybrid_plan.h -- host arithmetic of the MSD hybrid sort (sort_hybrid and
// sort_pieces_impl in radix_kernels.hip): the bucket blocks' size classes, the
// hybrid workspace block's layout, the words of its counters and host mirror,
// the host-side predicates and the piece table.  Pure C++17 with no HIP types
// (as distrib_plan.h): compiled into libsort.so and, with AddressSanitizer,
// into tests/cpp/hybrid_plan_test.cpp.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace lsort {
namespace hplan {

// ---- bucket classes ----
// The bucket sort's blocks come in two sizes: the first holds the mean bucket
// of uniform keys + 3.5 sigma (all but a few of the 65536 buckets), those few
// are listed for the second.  A row: threads per block, keys per thread of
// the first and of the second size.  Rows 0-3: 256-thread blocks (64-bit keys:
// the same slots in blocks of `bb` threads, keys per thread rounded up); row 4
// (32-bit keys): buckets of ~8K keys (sorts up to 2^29 + 2^23 keys); row 5
// (32-bit keys without values, the counting placement only): ~16K keys
// (2^30-key sorts).
struct BucketClass { int block, items1, items2; };
constexpr int kBucketClasses = 6;
constexpr BucketClass kBucketClass[kBucketClasses] = {{256, 9, 15},  {256, 13, 19}, {256, 17, 23},
                                                      {256, 19, 25}, {512, 17, 23}, {1024, 17, 23}};
// a row's block and keys per thread where the 256-thread rows run bb threads
constexpr int class_block(int cls, int bb) { return kBucketClass[cls].block == 256 ? bb : kBucketClass[cls].block; }
constexpr int class_items(int cls, int items, int bb) {
  return kBucketClass[cls].block == 256 ? (items * 256 + bb - 1) / bb : items;
}
constexpr int class_items1(int cls, int bb) { return class_items(cls, kBucketClass[cls].items1, bb); }
constexpr int class_items2(int cls, int bb) { return class_items(cls, kBucketClass[cls].items2, bb); }
// keys per thread of the 3-bit retry blocks over a 256-thread row's second size
constexpr int class_retry_items(int cls, int retry_block) {
  return (kBucketClass[cls].items2 * 256 + retry_block - 1) / retry_block;
}

// a range sort's keys lie in [bias, bias + span), span in (2^(W-1), 2^W]:
// only the first span / 2^(W-16) of the 16-bit prefixes (and span / 2^(W-BITS)
// of the top digits) are populated, each by n * 2^(W-16) / span keys on
// average (range rounds of the multi-GPU sort: a W = 27 round spans ~0.8 of
// 2^27, which the full-width shares would take for skew)
inline double range_fill(uint64_t span, int W) { return span ? (double)span / std::ldexp(1.0, W) : 1.0; }

struct BucketPlan {
  bool served;         // false: the LSD sort
  int cls, block;      // row of kBucketClass, threads per block
  uint32_t cap1, cap;  // slots of the first and the second size
  int retry_items;
  double mean, need;   // the mean bucket of uniform keys, + 3.5 sigma
};
// The row whose first size holds `need`; 64-bit keys stop at row 3; row 5 needs
// the counting placement and, as the last, must hold `need`, else not served.
inline BucketPlan bucket_plan(size_t n, uint32_t NB, double fill, int key_bytes, bool counting, int bb64,
                              int retry_block) {
  BucketPlan p{};
  p.mean = (double)n / (NB * fill);
  p.need = p.mean + 3.5 * std::sqrt(p.mean);
  const int bb = key_bytes == 8 ? bb64 : 256;
  const int last = key_bytes == 8 ? 3 : kBucketClasses - 1;
  int cls = 0;
  while (cls < last && p.need > (double)kBucketClass[cls].block * kBucketClass[cls].items1) ++cls;
  p.cls = cls;
  p.block = class_block(cls, bb);
  p.cap1 = (uint32_t)(p.block * class_items1(cls, bb));
  p.cap = (uint32_t)(p.block * class_items2(cls, bb));
  p.retry_items = class_retry_items(cls, retry_block);
  p.served = !(cls == 5 && (!counting || p.need > (double)p.cap1));
  return p;
}

// ---- the hybrid workspace block (Workspace::hyb), its counters, the host mirror ----
constexpr uint32_t kListCap = 1024;  // the listed buckets over the first size
constexpr int kRsvRanges = 8;        // reserved depth 0: ranges per digit (slices = children * ranges)
constexpr int kRsvBlocks = 32;       // sampling blocks per range

// words of ctr[]
enum : uint32_t {
  kCtrTiles = 0,      // [k]: tiles of depth k (k <= 4)
  kCtrLsdN2 = 7,      // kCnt2F: the LSD-step list after the 2-bit cells (flist2)
  kCtrOver1 = 8,      // buckets over the first size (olist)
  kCtrBuckets = 9,    // bucket count
  kCtrOver2 = 10,     // buckets over the second size
  kCtrStats = 11,     // [11..14] are mirrored to hyb_host[kHostStats..] by the last depth
  kCtrMaxBucket = 11, // largest bucket
  kCtrPlanOver1 = 12, // buckets over the first size (planning)
  kCtrMaxChild = 13,  // largest child of depth 0 (pieces)
  kCtrRsvOver = 14,   // reserved depth 0 overflowed (the list launches' unused over-count lands here, after the read)
  kCtrOvfN = 15,      // buckets whose counting placement overflowed (flist)
  kCtrWords = 16
};
// words of hyb_host[] (pinned, kHostWords)
enum : uint32_t {
  kHostDigits = 0,      // [0, RADIX): depth 0's digit sizes or starts (pieces, reserved: [0] the largest child)
  kHostStats = 256,     // ctr[kCtrStats..kCtrStats + 4) after the last depth
  kHostMaxBucket = kHostStats + kCtrMaxBucket - kCtrStats,
  kHostPlanOver1 = kHostStats + kCtrPlanOver1 - kCtrStats,
  kHostRsvOver = kHostStats + kCtrRsvOver - kCtrStats,
  kHostMaxChild = 260,  // pieces, counted depth 0: its largest child
  kHybSeqWord2 = 510,   // k_hyb_children's sequence word, raised after the bucket stats
  kHybSeqWord = 511,    // the samplers', raised after their size estimates (polled instead of an event)
  kHostWords = 512
};

// Offsets (u32 words) of the block's regions, in order: tiles[2] (uint4 per
// tile, 16-byte aligned) | segbase | cstart[2] | nsize | ctile0[2] | ntl | ctr
// | olist (buckets over the first size) | flist (counting placement overflowed)
// | flist2 (kCnt2F: for the LSD steps) | reserved depth 0: rpart (sample
// partials) | rslice (start | capacity | first tile, + the tile count).
struct HybLayout {
  size_t tiles[2], segbase, cstart[2], nsize, ctile0[2], ntl, ctr, olist, flist, flist2, rpart, rslice, words;
};
// TB: the most tiles of a depth; NB: buckets; rnc: children of depth 0
inline HybLayout hyb_layout(uint32_t TB, uint32_t NB, uint32_t rnc) {
  HybLayout L{};
  size_t w = 0;
  auto take = [&w](size_t k) { return (w += k) - k; };
  const size_t rns = (size_t)rnc * kRsvRanges;
  for (size_t& t : L.tiles) t = take((size_t)TB * 4);
  L.segbase = take(NB);
  for (size_t& c : L.cstart) c = take(NB);
  L.nsize = take(NB);
  for (size_t& c : L.ctile0) c = take((size_t)NB + 1);
  L.ntl = take(NB);
  L.ctr = take(kCtrWords);
  L.olist = take(kListCap);
  L.flist = take(NB);
  L.flist2 = take(NB);
  L.rpart = take((size_t)kRsvRanges * kRsvBlocks * rnc);
  L.rslice = take(3 * rns + 16);
  L.words = w;
  return L;
}

// ---- predicates ----
// mode (libsortSetHybridMode): 1 auto (min <= n <= max), 2 forced (1024 <= n <= max)
inline bool hybrid_serves(int mode, size_t n, size_t min, size_t max) {
  return (mode == 1 && n >= min && n <= max) || (mode == 2 && n >= 1024 && n <= max);
}

// Words of the reserved depth 0's slices: n keys plus each slice's sampled
// slack (k_rsv_sample: (s + 5 sqrt(s) + 24) N / S per slice, rounded up to
// whole tiles), over NS = nc * 8 slices, S samples per range: at most
// n (1 + 5 sqrt(nc / S) + 25 nc / S) + NS * TILE.
inline size_t rsv_capacity_bound_nc(size_t n, uint32_t nc, uint32_t S, uint32_t tile) {
  const double f = 5.0 * std::sqrt((double)nc / S) + 25.0 * nc / S;
  return n + (size_t)std::ceil((double)n * f) + (size_t)nc * kRsvRanges * tile + 1024;
}

// Tile rows of depth k over nseg_k segments: T0 at depth 0, the reserved
// slices' rows (tb1) after a reserved depth 0, else Tt + a partial tile each.
inline uint32_t tile_bound(int k, uint32_t T0, uint32_t Tt, uint32_t tb1, bool rsv, uint32_t nseg_k) {
  return k == 0 ? T0 : (k == 1 && rsv) ? tb1 : Tt + nseg_k;
}

// Where depth k reads its keys (and depth k - 1 wrote them): the last depth
// writes out, so depth k writes out when depths - 1 - k is even, tmp otherwise;
// depth 0 reads in; a reserved depth 0 writes the slices (keys only).
enum class Buf { In, Rsv, Tmp, Out };
inline Buf key_buf(int k, int depths, bool rsv) {
  return k == 0 ? Buf::In : (k == 1 && rsv) ? Buf::Rsv : ((depths - k) & 1) ? Buf::Tmp : Buf::Out;
}
inline Buf val_buf(int k, int depths) { return key_buf(k, depths, false); }

// pack16 needs a full-width sort of a whole array, the
// counting placement and the reserved depth 0 (rmode 1: not its test mode with
// short slices, whose overflow abandons the later depths).  The u16 array goes
// where neither the last pass reads nor out is: the slices, which depth 1 has
// consumed, or tmp when the last pass reads the slices (two depths).
inline bool pack16_eligible(bool pieces, int W, uint32_t lbits, bool counting, int rmode) {
  return !pieces && W == 32 && lbits == 16 && counting && rmode == 1;
}
inline Buf pack16_buf(int depths) { return depths >= 3 ? Buf::Rsv : Buf::Tmp; }

// Skew checks after depth 0.  A top digit of mx keys well above its share (beyond
// sampling noise), or whose buckets would average > 0.9 of a block: the LSD sort.
inline bool top_digit_skewed(uint32_t mx, size_t n, int radix, double fill, uint32_t NB, uint32_t cap) {
  const double share = (double)n / (radix * fill);
  return (double)mx > 1.25 * share + 4.0 * std::sqrt(share) + 32.0 || (double)mx / (double)(NB / radix) > 0.9 * cap;
}
// pieces: a depth-0 child of mx keys, split by bits_below more digit bits
inline bool piece_child_skewed(uint32_t mx, int bits_below, uint32_t cap) {
  return (double)mx / (double)(1ull << bits_below) > 0.9 * cap;
}

// ---- piece table (sort_pieces_u32) ----
// Piece p = keys in[off_p, off_p + len_p) of segment seg_p.  The table, one
// buffer: pieces uint4 (off, len, seg, first tile) | ctile0[nseg + 1] |
// cstart[nseg] | cum[K + 1] (keys before each piece) | (uint64 word g64) the
// fallback's gather table src_off[K] | dst_off[K] | len[K]; 24-bit pieces
// (planar): a 4th column, each piece's top byte << 24, then seghi[nseg] (u32).
// K: the non-empty pieces; nseg: the populated segments, renumbered in order.
struct PieceTable {
  bool ok;      // false: an invalid table
  uint32_t K, nseg, tiles;
  int depths;   // digit passes of the hybrid; 0: gather + LSD sort
  double fill;  // populated segments / nseg
  uint64_t maxlen;
  uint32_t first_seg, last_seg;        // of the non-empty pieces (caller's numbering)
  size_t ctile0, cstart, cum;          // u32 offsets
  size_t g64, gcols, seghi64, words;   // uint64 offsets and size
};
// Checks the table (segments non-decreasing and < nseg, offsets below 2^32,
// lengths summing to n, at most 65535 non-empty pieces), sizes it and fills
// the buffer get_buf(words) gives (null: returns unfilled).  hybrid: the hybrid
// may serve this sort; tile: keys per depth-0 tile; hi0: planar's first top byte.
template <typename GetBuf>
PieceTable piece_table(const uint64_t* off, const uint64_t* len, const uint32_t* seg, size_t np, uint32_t nseg,
                       size_t n, int bits, int digit_bits, bool hybrid, uint32_t tile, bool planar, uint32_t hi0,
                       GetBuf&& get_buf) {
  PieceTable t{};
  std::vector<size_t> keep;
  keep.reserve(np);
  uint64_t total = 0;
  uint32_t prev = 0;
  for (size_t p = 0; p < np; ++p) {
    if (seg[p] < prev || seg[p] >= nseg) return t;
    prev = seg[p];
    if (!len[p]) continue;
    if (off[p] + len[p] > 0xffffffffull) return t;
    total += len[p];
    t.maxlen = std::max(t.maxlen, len[p]);
    keep.push_back(p);
  }
  if (total != n || keep.size() > 65535) return t;
  t.ok = true;
  const uint32_t K = t.K = (uint32_t)keep.size();
  t.first_seg = K ? seg[keep[0]] : 0;
  t.last_seg = K ? seg[keep[K - 1]] : 0;
  // segment sizes: the largest sets the digit passes, the populated ones the
  // bucket blocks' size class (a round's last group may span many empty
  // digits)
  std::vector<uint64_t> segsize(nseg, 0);
  for (size_t p : keep) segsize[seg[p]] += len[p];
  uint64_t maxseg = 0;
  uint32_t npop = 0;
  // the populated segments only, renumbered in order (empty segments hold no
  // keys, so the output order is unchanged; a round over many empty digits
  // would otherwise launch a bucket block per empty bucket: 2^29 keys in the
  // 8-GPU shape, a round of 233 digits with 9 populated, ~0.7 ms of empty
  // blocks)
  std::vector<uint32_t> cseg(nseg, 0);
  for (uint32_t s = 0; s < nseg; ++s) {
    maxseg = std::max(maxseg, segsize[s]);
    cseg[s] = npop;
    if (segsize[s]) segsize[npop++] = segsize[s];
  }
  segsize.resize(npop);
  nseg = t.nseg = npop;
  t.fill = 1.0;  // (every renumbered segment is populated)
  // digit passes: the fewest that bring the largest segment's mean bucket
  // (its keys / RADIX^d, values uniform within a segment) to <= 8320 keys
  // (the 512 x 17-key block holds that + 3.5 sigma), within `bits`
  if (bits > 0 && hybrid) {
    for (int d = 1; d * digit_bits <= bits; ++d) {
      t.depths = d;
      if ((double)maxseg / std::ldexp(1.0, d * digit_bits) <= 8320.0) break;
    }
    if (((uint64_t)nseg << (digit_bits * t.depths)) > (1ull << 22)) t.depths = 0;
  }
  t.ctile0 = 4 * (size_t)K;
  t.cstart = t.ctile0 + nseg + 1;
  t.cum = t.cstart + nseg;
  t.g64 = (t.cum + (size_t)K + 1 + 1) / 2;
  t.gcols = planar ? 4 : 3;
  t.seghi64 = t.g64 + t.gcols * (size_t)K;
  t.words = t.seghi64 + (planar ? ((size_t)nseg + 1) / 2 : 0);
  uint64_t* const buf = get_buf(t.words);
  if (!buf) return t;
  uint32_t* const h32 = reinterpret_cast<uint32_t*>(buf);
  uint32_t *const ct0 = h32 + t.ctile0, *const cst = h32 + t.cstart, *const pcum = h32 + t.cum;
  uint64_t* const hg = buf + t.g64;
  {
    uint64_t run = 0;
    for (uint32_t s = 0; s < nseg; ++s) {
      cst[s] = (uint32_t)run;
      run += segsize[s];
    }
  }
  uint32_t tl = 0, i = 0, run = 0;
  std::vector<uint64_t> dpos(cst, cst + nseg);
  for (uint32_t s = 0; s <= nseg; ++s) {
    ct0[s] = tl;  // segment s's pieces start at this tile
    for (; i < K && (s == nseg || cseg[seg[keep[i]]] == s); ++i) {
      const size_t p = keep[i];
      const uint32_t cs = cseg[seg[p]];
      pcum[i] = run;
      run += (uint32_t)len[p];
      h32[4 * (size_t)i + 0] = (uint32_t)off[p];
      h32[4 * (size_t)i + 1] = (uint32_t)len[p];
      h32[4 * (size_t)i + 2] = cs;
      h32[4 * (size_t)i + 3] = tl;
      tl += (uint32_t)((len[p] + tile - 1) / tile);
      hg[i] = off[p];
      hg[K + i] = dpos[cs];
      hg[2 * (size_t)K + i] = len[p];
      if (planar) hg[3 * (size_t)K + i] = (uint64_t)(hi0 + seg[p]) << 24;
      dpos[cs] += len[p];
    }
  }
  pcum[K] = run;
  t.tiles = tl;
  uint32_t* shi = reinterpret_cast<uint32_t*>(buf + t.seghi64);
  if (planar)
    for (uint32_t i2 = 0; i2 < K; ++i2) shi[cseg[seg[keep[i2]]]] = (hi0 + seg[keep[i2]]) << 24;
  return t;
}

}  // namespace hplan
}  // namespace lsort
