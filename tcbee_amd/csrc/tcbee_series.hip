// tcbee_series.hip — per-flow TCP series analysis of a flow-major batch on the device
// (DESIGN.md "Per-flow series"): sequence / acknowledgement numbers unwrapped relative
// to each flow's first record, the marks (below the high-water mark, repeated pair,
// first of its flow) and one summary row per flow. Everything is a segmented scan or a
// segmented reduction over the columns tcbee_group_by_flow_device leaves in HBM.
// Context-free like tcbee_group.hip: the caller owns every buffer, nothing is
// allocated, nothing synchronises, and no kernel waits on another workgroup — order
// between the steps comes from the launches on the stream alone.
//
//   k_series_clear   zero the head bitmap (a kernel, so the call can be captured)
//   k_series_heads   one lane per segment: its stats row, its head bit
//   k_series_reduce  per tile of kSerTile positions: the tile's aggregate
//   k_series_carry   one workgroup: exclusive segmented scan of the aggregates, in place
//   k_series_apply   per tile: rescan with the carry-in, outputs, per-run atomics
// (block_excl and series_segment: tcbee_scan.h)
#include "tcbee_scan.h"
#include "tcbee_table.h"

namespace tcbee {

constexpr uint32_t kSerBlock = 256;
constexpr uint32_t kSerWaves = kSerBlock / 64;
constexpr uint32_t kSerItems = 8;                       // consecutive records per lane
constexpr uint32_t kSerTile = kSerBlock * kSerItems;    // 2048 (series.SERIES_TILE)
constexpr uint32_t kCarryBlock = 1024;
constexpr uint32_t kCarryWaves = kCarryBlock / 64;
constexpr uint32_t kCarryItems = 4;                     // tiles per lane and round
static_assert(kSerItems == 8, "a lane's head flags are one byte of the bitmap");

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

// The max-prefix-sum monoid of both columns, lifted to segments: s = sum of the
// differences, m = max(0, largest prefix sum), f = "holds a head". m >= s and m >= 0
// always, so {0, 0} is the identity on both sides.
struct Rel {
  int64_t s1, m1, s2, m2;
  uint32_t f;
};
__device__ __forceinline__ Rel rel_id() { return Rel{0, 0, 0, 0, 0u}; }
__device__ __forceinline__ int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }
__device__ __forceinline__ Rel combine(const Rel& l, const Rel& r) {
  if (r.f) return r;  // a right operand that holds a head replaces the left
  return Rel{l.s1 + r.s1, max64(l.m1, l.s1 + r.m1), l.s2 + r.s2, max64(l.m2, l.s2 + r.m2), l.f};
}
__device__ __forceinline__ Rel shfl_up_v(const Rel& x, uint32_t o) {
  return Rel{(int64_t)__shfl_up((long long)x.s1, o), (int64_t)__shfl_up((long long)x.m1, o),
             (int64_t)__shfl_up((long long)x.s2, o), (int64_t)__shfl_up((long long)x.m2, o),
             __shfl_up(x.f, o)};
}

// What a run (the part of a segment inside one tile) adds to its stats row. cnt packs
// four counts of at most kSerTile each in 16-bit fields: seq below, ack below, repeat,
// zero window. Every component combines exactly in any order.
struct Run {
  uint64_t cnt, gap;
  uint32_t wmin, wmax, fl, f;
};
__device__ __forceinline__ Run run_id() { return Run{0ull, 0ull, 0xFFFFu, 0u, 0u, 0u}; }
__device__ __forceinline__ Run combine(const Run& l, const Run& r) {
  if (r.f) return r;
  return Run{l.cnt + r.cnt, l.gap > r.gap ? l.gap : r.gap, l.wmin < r.wmin ? l.wmin : r.wmin,
             l.wmax > r.wmax ? l.wmax : r.wmax, l.fl | r.fl, l.f};
}
__device__ __forceinline__ Run shfl_up_v(const Run& x, uint32_t o) {
  return Run{(uint64_t)__shfl_up((unsigned long long)x.cnt, o),
             (uint64_t)__shfl_up((unsigned long long)x.gap, o), __shfl_up(x.wmin, o),
             __shfl_up(x.wmax, o), __shfl_up(x.fl, o), __shfl_up(x.f, o)};
}
static_assert(kSerTile < (1u << 16), "Run::cnt holds four 16-bit counts");

struct SeriesArgs {
  tcbee_series_in in;
  tcbee_series_out out;
  uint32_t* bitmap;  // bit j: position j is the first of a non-empty segment
  uint64_t* agg;     // [tiles][6]: s1 m1 s2 m2 f -, the carry-in of a tile after k_series_carry
  uint32_t n_max, n_ids;
};

__device__ __forceinline__ uint32_t series_n(const SeriesArgs& a) {
  const uint32_t n = a.in.flow_start[a.n_ids + 1u];
  return n < a.n_max ? n : a.n_max;
}

__device__ __forceinline__ Rel agg_load(const uint64_t* p) {
  const u64x2 a = *reinterpret_cast<const u64x2*>(p), b = *reinterpret_cast<const u64x2*>(p + 2),
              c = *reinterpret_cast<const u64x2*>(p + 4);
  return Rel{(int64_t)a.x, (int64_t)a.y, (int64_t)b.x, (int64_t)b.y, (uint32_t)c.x};
}
__device__ __forceinline__ void agg_store(uint64_t* p, const Rel& r) {
  *reinterpret_cast<u64x2*>(p) = u64x2{(uint64_t)r.s1, (uint64_t)r.m1};
  *reinterpret_cast<u64x2*>(p + 2) = u64x2{(uint64_t)r.s2, (uint64_t)r.m2};
  *reinterpret_cast<u64x2*>(p + 4) = u64x2{(uint64_t)r.f, 0ull};
}

__global__ __launch_bounds__(kSerBlock) void k_series_clear(u32x4* bitmap, uint32_t vecs) {
  const uint32_t i = blockIdx.x * kSerBlock + threadIdx.x;
  if (i < vecs) bitmap[i] = u32x4{0u, 0u, 0u, 0u};
}

// ---------------------------------------------------------------------------
// Heads: lane k owns segment k. Its row gets the plain fields and the identities
// of the ones the apply kernel accumulates; its first position gets its head bit.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kSerBlock) void k_series_heads(SeriesArgs a) {
  const uint32_t k = blockIdx.x * kSerBlock + threadIdx.x;
  if (k > a.n_ids) return;
  const uint32_t n = series_n(a);
  uint32_t lo = a.in.flow_start[k], hi = a.in.flow_start[k + 1u];
  lo = lo < n ? lo : n;
  hi = hi < n ? hi : n;
  const bool some = hi > lo;
  if (some) atomicOr(&a.bitmap[lo >> 5], 1u << (lo & 31u));
  if (a.out.stats) {
    uint64_t* const row = reinterpret_cast<uint64_t*>(a.out.stats + k);
    row[0] = some ? a.in.ts_ns[lo] : 0ull;
    row[1] = some ? a.in.ts_ns[hi - 1u] : 0ull;
    row[2] = row[3] = row[4] = 0ull;          // spans, max_gap
    row[5] = some ? (uint64_t)(hi - lo) : 0ull;  // records, n_seq_below
    row[6] = 0ull;                            // n_ack_below, n_repeat
    row[7] = 0xFFFFull << 32;                 // n_zero_window, win_min
    row[8] = 0ull;                            // win_max, flags_or
  }
}

// ---------------------------------------------------------------------------
// A lane's eight positions: the 32-bit differences of both columns (0 at a head and at
// or past n), the head and validity masks. Lane l of the workgroup holds positions
// tbase + 8 l .. + 7, loaded as two 16-byte vectors per column; the value before the
// lane's first comes from the lane below, for a wave's first lane from memory.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void load8(const uint32_t* p, uint32_t g0, uint32_t n, uint32_t (&v)[8]) {
  if (g0 + kSerItems <= n) {
    const u32x4 x = *reinterpret_cast<const u32x4*>(p + g0);
    const u32x4 y = *reinterpret_cast<const u32x4*>(p + g0 + 4);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    v[4] = y.x; v[5] = y.y; v[6] = y.z; v[7] = y.w;
  } else {
#pragma unroll
    for (uint32_t i = 0; i < kSerItems; ++i) v[i] = g0 + i < n ? p[g0 + i] : 0u;
  }
}

struct Lane {
  uint32_t g0, valid, heads;  // bit i: position g0 + i is below n / is a head
  int32_t d1[kSerItems], d2[kSerItems];
};

__device__ __forceinline__ void lane_load(const SeriesArgs& a, uint32_t n, uint32_t tbase, Lane& L) {
  const uint32_t lane = threadIdx.x & 63u;
  L.g0 = tbase + threadIdx.x * kSerItems;
  const uint32_t left = L.g0 < n ? n - L.g0 : 0u;
  L.valid = left >= kSerItems ? 0xFFu : (1u << left) - 1u;
  uint32_t s[kSerItems], k[kSerItems];
  load8(a.in.seq, L.g0, n, s);
  load8(a.in.ack, L.g0, n, k);
  L.heads = left ? reinterpret_cast<const uint8_t*>(a.bitmap)[L.g0 >> 3] & L.valid : 0u;
  uint32_t ps = __shfl_up(s[kSerItems - 1], 1), pk = __shfl_up(k[kSerItems - 1], 1);
  if (lane == 0) {
    const bool has = left && L.g0 > 0;
    ps = has ? a.in.seq[L.g0 - 1u] : 0u;
    pk = has ? a.in.ack[L.g0 - 1u] : 0u;
  }
#pragma unroll
  for (uint32_t i = 0; i < kSerItems; ++i) {
    const bool live = ((L.valid & ~L.heads) >> i) & 1u;
    L.d1[i] = live ? (int32_t)(s[i] - (i ? s[i - 1] : ps)) : 0;
    L.d2[i] = live ? (int32_t)(k[i] - (i ? k[i - 1] : pk)) : 0;
  }
}

// one position appended to a running state (combine with (d, max(d, 0)))
__device__ __forceinline__ void rel_step(Rel& r, bool head, int32_t d1, int32_t d2) {
  if (head) {
    r = Rel{0, 0, 0, 0, 1u};
  } else {
    r.s1 += d1; r.m1 = max64(r.m1, r.s1);
    r.s2 += d2; r.m2 = max64(r.m2, r.s2);
  }
}

__device__ __forceinline__ Rel lane_reduce(const Lane& L) {
  Rel r = rel_id();
#pragma unroll
  for (uint32_t i = 0; i < kSerItems; ++i) rel_step(r, (L.heads >> i) & 1u, L.d1[i], L.d2[i]);
  return r;
}

// ---------------------------------------------------------------------------
// Reduce: the tile's aggregate, from its last head (its start if it has none) to its end.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kSerBlock) void k_series_reduce(SeriesArgs a) {
  const uint32_t n = series_n(a);
  const uint32_t tile = blockIdx.x, tbase = tile * kSerTile;
  if (tbase >= n) return;
  __shared__ Rel s_w[kSerWaves];
  Lane L;
  lane_load(a, n, tbase, L);
  Rel total;
  (void)block_excl<kSerWaves>(lane_reduce(L), rel_id(), s_w, total);
  if (threadIdx.x == 0) agg_store(a.agg + 6ull * tile, total);
}

// ---------------------------------------------------------------------------
// Carry: one workgroup turns the aggregates of tiles [0, ceil(n / kSerTile)) into their
// exclusive segmented scan, in place: agg[t] becomes the state at the end of tile t - 1.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kCarryBlock) void k_series_carry(SeriesArgs a) {
  const uint32_t n = series_n(a);
  const uint32_t ntiles = (n + kSerTile - 1u) / kSerTile;
  __shared__ Rel s_w[kCarryWaves];
  Rel carry = rel_id();
  for (uint32_t t0 = 0; t0 < ntiles; t0 += kCarryBlock * kCarryItems) {
    const uint32_t t = t0 + threadIdx.x * kCarryItems;
    Rel c[kCarryItems], sum = rel_id();
#pragma unroll
    for (uint32_t i = 0; i < kCarryItems; ++i) {
      c[i] = t + i < ntiles ? agg_load(a.agg + 6ull * (t + i)) : rel_id();
      sum = combine(sum, c[i]);
    }
    Rel total;
    Rel x = combine(carry, block_excl<kCarryWaves>(sum, rel_id(), s_w, total));
#pragma unroll
    for (uint32_t i = 0; i < kCarryItems; ++i) {
      if (t + i < ntiles) agg_store(a.agg + 6ull * (t + i), x);
      x = combine(x, c[i]);
    }
    carry = combine(carry, total);
  }
}

// ---------------------------------------------------------------------------
// Apply: the tile again with its carry-in. REL: seq_rel or ack_rel is wanted; STATS: the
// rows are (then ts_ns / window / flags are read and the runs' atomics issued).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void store8(int64_t* p, const Lane& L, const int64_t (&v)[kSerItems]) {
  if (L.valid == 0xFFu) {
#pragma unroll
    for (uint32_t i = 0; i < kSerItems; i += 2)
      *reinterpret_cast<u64x2*>(p + L.g0 + i) = u64x2{(uint64_t)v[i], (uint64_t)v[i + 1]};
  } else {
#pragma unroll
    for (uint32_t i = 0; i < kSerItems; ++i)
      if ((L.valid >> i) & 1u) p[L.g0 + i] = v[i];
  }
}

template <bool REL, bool STATS>
__global__ __launch_bounds__(kSerBlock) void k_series_apply(SeriesArgs a) {
  const uint32_t n = series_n(a);
  const uint32_t tile = blockIdx.x, tbase = tile * kSerTile;
  if (tbase >= n) return;
  __shared__ Rel s_w[kSerWaves];
  __shared__ Run s_r[kSerWaves];
  Lane L;
  lane_load(a, n, tbase, L);
  Rel unused;
  const Rel pre = combine(agg_load(a.agg + 6ull * tile),
                          block_excl<kSerWaves>(lane_reduce(L), rel_id(), s_w, unused));

  // marks, and the unwrapped values as they pass
  uint32_t mk[kSerItems];
  {
    Rel r = pre;
    int64_t v1[kSerItems], v2[kSerItems];
#pragma unroll
    for (uint32_t i = 0; i < kSerItems; ++i) {
      const bool head = (L.heads >> i) & 1u;
      const int64_t h1 = r.m1, h2 = r.m2;  // the high-water marks before this position
      rel_step(r, head, L.d1[i], L.d2[i]);
      mk[i] = head ? 8u
                   : (r.s1 < h1 ? 1u : 0u) | (r.s2 < h2 ? 2u : 0u) |
                         ((L.d1[i] | L.d2[i]) == 0 ? 4u : 0u);
      if (!((L.valid >> i) & 1u)) mk[i] = 0u;
      v1[i] = r.s1;
      v2[i] = r.s2;
    }
    if (REL && a.out.seq_rel) store8(a.out.seq_rel, L, v1);
    if (REL && a.out.ack_rel) store8(a.out.ack_rel, L, v2);
  }
  if (a.out.mark) {
    const u32x2 m{mk[0] | mk[1] << 8 | mk[2] << 16 | mk[3] << 24,
                  mk[4] | mk[5] << 8 | mk[6] << 16 | mk[7] << 24};
    if (L.valid == 0xFFu) {
      *reinterpret_cast<u32x2*>(a.out.mark + L.g0) = m;
    } else {
#pragma unroll
      for (uint32_t i = 0; i < kSerItems; ++i)
        if ((L.valid >> i) & 1u) a.out.mark[L.g0 + i] = (uint8_t)mk[i];
    }
  }
  if (!STATS) return;

  // what each position adds to its run
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t left = n - (L.g0 < n ? L.g0 : n);
  uint64_t ts[kSerItems];
  uint32_t win[kSerItems], fl[kSerItems];
  if (L.valid == 0xFFu) {
#pragma unroll
    for (uint32_t i = 0; i < kSerItems; i += 2) {
      const u64x2 t = *reinterpret_cast<const u64x2*>(a.in.ts_ns + L.g0 + i);
      ts[i] = t.x;
      ts[i + 1] = t.y;
    }
    const u32x4 w = *reinterpret_cast<const u32x4*>(a.in.window + L.g0);
    const u32x2 f = *reinterpret_cast<const u32x2*>(a.in.flags + L.g0);
    const uint32_t wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (uint32_t i = 0; i < kSerItems; ++i) {
      win[i] = (wv[i >> 1] >> (16u * (i & 1u))) & 0xFFFFu;
      fl[i] = ((i < 4 ? f.x : f.y) >> (8u * (i & 3u))) & 0xFFu;
    }
  } else {
#pragma unroll
    for (uint32_t i = 0; i < kSerItems; ++i) {
      const bool ok = (L.valid >> i) & 1u;
      ts[i] = ok ? a.in.ts_ns[L.g0 + i] : 0ull;
      win[i] = ok ? a.in.window[L.g0 + i] : 0u;
      fl[i] = ok ? a.in.flags[L.g0 + i] : 0u;
    }
  }
  uint64_t pt = (uint64_t)__shfl_up((unsigned long long)ts[kSerItems - 1], 1);
  if (lane == 0) pt = left && L.g0 > 0 ? a.in.ts_ns[L.g0 - 1u] : 0ull;
  auto item = [&](uint32_t i) {  // (made twice from the registers, not kept)
    if (!((L.valid >> i) & 1u)) return run_id();
    const uint64_t before = i ? ts[i ? i - 1 : 0] : pt;
    const bool head = (L.heads >> i) & 1u;
    return Run{(uint64_t)(mk[i] & 1u) | (uint64_t)((mk[i] >> 1) & 1u) << 16 |
                   (uint64_t)((mk[i] >> 2) & 1u) << 32 | (uint64_t)(win[i] == 0u) << 48,
               !head && ts[i] >= before ? ts[i] - before : 0ull, win[i], win[i], fl[i], 0u};
  };
  Run sum = run_id();
#pragma unroll
  for (uint32_t i = 0; i < kSerItems; ++i) {
    if ((L.heads >> i) & 1u) sum = Run{0ull, 0ull, 0xFFFFu, 0u, 0u, 1u};
    sum = combine(sum, item(i));
  }
  Run total;
  Run run = block_excl<kSerWaves>(sum, run_id(), s_r, total);

  // a run ends where the next position is a head, at n - 1 and at the tile's end; a
  // segment ends at the first two
  const uint32_t next = left > kSerItems
                            ? reinterpret_cast<const uint8_t*>(a.bitmap)[(L.g0 >> 3) + 1u] & 1u
                            : 1u;
  const uint32_t seg_tail = L.valid & (((L.heads | next << 8) >> 1) | ((~L.valid & 0xFFu) >> 1));
  const uint32_t run_tail = seg_tail | (threadIdx.x == kSerBlock - 1u ? L.valid & 0x80u : 0u);
  if (run_tail == 0u) return;
  Rel r = pre;
#pragma unroll
  for (uint32_t i = 0; i < kSerItems; ++i) {
    const bool head = (L.heads >> i) & 1u;
    rel_step(r, head, L.d1[i], L.d2[i]);
    if (head) run = run_id();
    run = combine(run, item(i));
    if (!((run_tail >> i) & 1u)) continue;
    tcbee_flow_stats* const row = a.out.stats + series_segment(a.in.flow_start, a.n_ids, L.g0 + i);
    if ((seg_tail >> i) & 1u) {
      row->seq_span = r.m1;
      row->ack_span = r.m2;
    }
    const uint32_t c0 = run.cnt & 0xFFFFu, c1 = (run.cnt >> 16) & 0xFFFFu,
                   c2 = (run.cnt >> 32) & 0xFFFFu, c3 = (run.cnt >> 48) & 0xFFFFu;
    if (c0) atomicAdd(&row->n_seq_below, c0);
    if (c1) atomicAdd(&row->n_ack_below, c1);
    if (c2) atomicAdd(&row->n_repeat, c2);
    if (c3) atomicAdd(&row->n_zero_window, c3);
    if (run.gap) atomicMax(reinterpret_cast<unsigned long long*>(&row->max_gap_ns),
                           (unsigned long long)run.gap);
    if (run.wmin < 0xFFFFu) atomicMin(&row->win_min, run.wmin);
    if (run.wmax) atomicMax(&row->win_max, run.wmax);
    if (run.fl) atomicOr(&row->flags_or, run.fl);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {

int series_err(hipError_t e) {
  if (e == hipSuccess) return TCBEE_OK;
  if (e == hipErrorOutOfMemory) return TCBEE_ENOMEM;
  if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return TCBEE_ENODEV;
  return TCBEE_EDEVICE;
}
#define TRY_HIP(expr)                             \
  do {                                            \
    hipError_t e_ = (expr);                       \
    if (e_ != hipSuccess) return series_err(e_);  \
  } while (0)

constexpr uint64_t kSeriesMaxRecords = 1ull << 31;  // n_max below it: u32 positions

bool series_args_ok(uint64_t n_max, uint64_t n_ids) {
  return n_ids >= 1 && n_ids <= kMaxTableFlows && n_max < kSeriesMaxRecords;
}

// Scratch: the head bitmap (one bit per position, whole 16-byte vectors, one vector to
// spare) and then 48 bytes per tile.
struct SeriesLayout {
  uint64_t bitmap_vecs, ntiles, bytes;
};
SeriesLayout series_layout(uint64_t n_max) {
  SeriesLayout l;
  l.bitmap_vecs = (n_max + 127) / 128 + 1;
  l.ntiles = (n_max + kSerTile - 1) / kSerTile;
  l.bytes = 16 * l.bitmap_vecs + 48 * l.ntiles;
  return l;
}

bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

}  // namespace
}  // namespace tcbee

using namespace tcbee;

extern "C" {

static_assert(sizeof(tcbee_flow_stats) == 72, "tcbee_flow_stats is 72 bytes");

uint64_t tcbee_series_scratch_bytes(uint64_t n_max, uint64_t n_ids) {
  if (!series_args_ok(n_max, n_ids)) return 0;
  return series_layout(n_max).bytes;
}

int tcbee_flow_series_device(const tcbee_series_in* in, uint64_t n_max, uint64_t n_ids,
                             const tcbee_series_out* out, void* scratch_dev,
                             uint64_t scratch_bytes, void* stream) {
  if (!in || !out || !in->flow_start || !in->seq || !in->ack || !scratch_dev) return TCBEE_EINVAL;
  if (out->stats && (!in->ts_ns || !in->window || !in->flags)) return TCBEE_EINVAL;
  if (!out->seq_rel && !out->ack_rel && !out->mark && !out->stats) return TCBEE_EINVAL;
  if (!series_args_ok(n_max, n_ids)) return TCBEE_EINVAL;
  if (scratch_bytes < tcbee_series_scratch_bytes(n_max, n_ids)) return TCBEE_EINVAL;
  if (misaligned16(in->seq) || misaligned16(in->ack) || misaligned16(in->ts_ns) ||
      misaligned16(in->window) || misaligned16(in->flags) || misaligned16(out->seq_rel) ||
      misaligned16(out->ack_rel) || misaligned16(out->mark) || misaligned16(scratch_dev))
    return TCBEE_EINVAL;
  if ((reinterpret_cast<uintptr_t>(in->flow_start) & 3u) || (reinterpret_cast<uintptr_t>(out->stats) & 7u))
    return TCBEE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const SeriesLayout l = series_layout(n_max);

  SeriesArgs a{};
  a.in = *in;
  a.out = *out;
  a.bitmap = static_cast<uint32_t*>(scratch_dev);
  a.agg = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(scratch_dev) + 16 * l.bitmap_vecs);
  a.n_max = (uint32_t)n_max;
  a.n_ids = (uint32_t)n_ids;
  if (!out->stats) a.in.ts_ns = nullptr, a.in.window = nullptr, a.in.flags = nullptr;

  const unsigned gc = (unsigned)((l.bitmap_vecs + kSerBlock - 1) / kSerBlock);
  hipLaunchKernelGGL(k_series_clear, dim3(gc), dim3(kSerBlock), 0, s,
                     reinterpret_cast<u32x4*>(a.bitmap), (uint32_t)l.bitmap_vecs);
  const unsigned gh = (unsigned)((n_ids + 1 + kSerBlock - 1) / kSerBlock);
  hipLaunchKernelGGL(k_series_heads, dim3(gh), dim3(kSerBlock), 0, s, a);
  const unsigned ntiles = (unsigned)l.ntiles;
  if (ntiles > 0) {
    hipLaunchKernelGGL(k_series_reduce, dim3(ntiles), dim3(kSerBlock), 0, s, a);
    hipLaunchKernelGGL(k_series_carry, dim3(1), dim3(kCarryBlock), 0, s, a);
    const bool rel = out->seq_rel || out->ack_rel;
    if (rel && out->stats) {
      hipLaunchKernelGGL((k_series_apply<true, true>), dim3(ntiles), dim3(kSerBlock), 0, s, a);
    } else if (rel) {
      hipLaunchKernelGGL((k_series_apply<true, false>), dim3(ntiles), dim3(kSerBlock), 0, s, a);
    } else if (out->stats) {
      hipLaunchKernelGGL((k_series_apply<false, true>), dim3(ntiles), dim3(kSerBlock), 0, s, a);
    } else {
      hipLaunchKernelGGL((k_series_apply<false, false>), dim3(ntiles), dim3(kSerBlock), 0, s, a);
    }
  }
  TRY_HIP(hipGetLastError());
  return TCBEE_OK;
}

int tcbee_flow_series(int device, const tcbee_series_in* in_host, uint64_t n, uint64_t n_ids,
                      const tcbee_series_out* out_host) {
  if (!in_host || !out_host || !in_host->flow_start) return TCBEE_EINVAL;
  if (n && (!in_host->seq || !in_host->ack)) return TCBEE_EINVAL;
  if (out_host->stats && n && (!in_host->ts_ns || !in_host->window || !in_host->flags))
    return TCBEE_EINVAL;
  if (!out_host->seq_rel && !out_host->ack_rel && !out_host->mark && !out_host->stats)
    return TCBEE_EINVAL;
  if (!series_args_ok(n, n_ids)) return TCBEE_EINVAL;
  TRY_HIP(hipSetDevice(device));
  // one allocation, cut into 16-byte aligned parts: scratch, six inputs, four outputs
  const bool st = out_host->stats != nullptr;
  const void* const hin[6] = {in_host->flow_start, in_host->seq, in_host->ack,
                              st ? in_host->ts_ns : nullptr, st ? in_host->window : nullptr,
                              st ? in_host->flags : nullptr};
  void* const hout[4] = {out_host->seq_rel, out_host->ack_rel, out_host->mark, out_host->stats};
  const uint64_t in_b[6] = {4 * (n_ids + 2), 4 * n, 4 * n, 8 * n, 2 * n, n};
  const uint64_t out_b[4] = {8 * n, 8 * n, n, sizeof(tcbee_flow_stats) * (n_ids + 1)};
  auto pad = [](uint64_t b) { return (b + 31) & ~15ull; };
  const uint64_t scr_b = pad(tcbee_series_scratch_bytes(n, n_ids));
  uint64_t in_off[6], out_off[4], total = scr_b;
  for (int k = 0; k < 6; ++k) {
    in_off[k] = total;
    if (k < 3 || st) total += pad(in_b[k]);  // (seq and ack get an address even when n == 0)
  }
  for (int k = 0; k < 4; ++k) {
    out_off[k] = total;
    if (hout[k]) total += pad(out_b[k]);
  }
  uint8_t* d = nullptr;
  TRY_HIP(hipMalloc(reinterpret_cast<void**>(&d), total));
  hipStream_t s = nullptr;
  int rc = TCBEE_OK;
  auto step = [&](hipError_t e) {
    if (rc == TCBEE_OK) rc = series_err(e);
    return rc == TCBEE_OK;
  };
  if (step(hipStreamCreateWithFlags(&s, hipStreamNonBlocking))) {
    for (int k = 0; k < 6; ++k)
      if (hin[k] && in_b[k]) step(hipMemcpyAsync(d + in_off[k], hin[k], in_b[k], hipMemcpyHostToDevice, s));
    tcbee_series_in di{};
    di.flow_start = reinterpret_cast<const uint32_t*>(d + in_off[0]);
    di.seq = reinterpret_cast<const uint32_t*>(d + in_off[1]);
    di.ack = reinterpret_cast<const uint32_t*>(d + in_off[2]);
    if (st) {
      di.ts_ns = reinterpret_cast<const uint64_t*>(d + in_off[3]);
      di.window = reinterpret_cast<const uint16_t*>(d + in_off[4]);
      di.flags = d + in_off[5];
    }
    tcbee_series_out dout{};
    if (hout[0]) dout.seq_rel = reinterpret_cast<int64_t*>(d + out_off[0]);
    if (hout[1]) dout.ack_rel = reinterpret_cast<int64_t*>(d + out_off[1]);
    if (hout[2]) dout.mark = d + out_off[2];
    if (hout[3]) dout.stats = reinterpret_cast<tcbee_flow_stats*>(d + out_off[3]);
    if (rc == TCBEE_OK) rc = tcbee_flow_series_device(&di, n, n_ids, &dout, d, scr_b, s);
    for (int k = 0; k < 4 && rc == TCBEE_OK; ++k)
      if (hout[k] && out_b[k])
        step(hipMemcpyAsync(hout[k], d + out_off[k], out_b[k], hipMemcpyDeviceToHost, s));
    // (also after an error: nothing of this call is left running when d is freed)
    step(hipStreamSynchronize(s));
    (void)hipStreamDestroy(s);
  }
  (void)hipFree(d);
  return rc;
}

}  // extern "C"
