// tcbee_peer.hip — a flow joined with its reverse direction on the device (DESIGN.md
// "Peer join"): which flow is the mirror of which, and per record the peer's cumulative
// acknowledgement (una), the upper edge of its advertised window and a round-trip sample,
// all rebuilt from the packets of one flow-major batch. The order between the two
// directions is perm's (capture order, no ties); the definitions are in
// include/tcbee_amd.h. Context-free like tcbee_series.hip: the caller owns every buffer,
// nothing is allocated, nothing synchronises, no kernel waits on another workgroup and
// every launch is a kernel.
//
//   k_peers_clear / insert / probe   an open-addressing table of ids by flow_hash64 in
//                                    scratch; probed with the mirrored tuple, full compare
//   k_peer_rows    one lane per segment: its stats row's identity
//   k_peer_rank    per tile: q (rank of each record among the peer's) and A (what it
//                  acknowledges, in the peer's frame) to scratch; the tile's max-aggregate
//   k_peer_carry   one workgroup: exclusive segmented max-scan of the aggregates
//   k_peer_scan    per tile: A -> H in place, the segmented running maximum
//   k_peer_apply   per tile: the peer's H and window at c + q - 1, the search for the
//                  acknowledging record, outputs, per-run atomics
//
// Searches. q and the acknowledging record rise along a segment, so a lane gallops
// from its previous answer. A tile that lies inside one segment (a hot flow: the deepest
// searches) finds its first position's rank once, stages the next kPeerLdsSlots entries
// of the peer's perm (rank) or H (apply) in LDS, and its lanes search there; an answer
// past the staged slice is searched in global memory from the slice's end.
#include "tcbee_scan.h"
#include "tcbee_table.h"
#if TCBEE_VARIANTS
#include <cstdlib>
#endif

namespace tcbee {

constexpr uint32_t kPeerBlock = 256;
constexpr uint32_t kPeerWaves = kPeerBlock / 64;
constexpr uint32_t kPeerItems = 8;                        // consecutive records per lane
constexpr uint32_t kPeerTile = kPeerBlock * kPeerItems;   // 2048, the series tile
constexpr uint32_t kPeerLdsSlots = 4096;                  // peer.PEER_LDS_SLOTS: 16 KB of perm, 32 KB of H
constexpr uint32_t kPeerCarryBlock = 1024;
constexpr uint32_t kPeerCarryWaves = kPeerCarryBlock / 64;
constexpr uint32_t kPeerCarryItems = 4;
constexpr uint32_t kNoPeer = TCBEE_NO_PEER;
constexpr int64_t kNone = INT64_MIN;
static_assert(kPeerItems == 8, "a lane's head flags are one byte");

typedef uint32_t pu32x2 __attribute__((ext_vector_type(2)));
typedef uint64_t pu64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umax32(uint32_t a, uint32_t b) { return a > b ? a : b; }

// ---------------------------------------------------------------------------
// Pairing
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t peer_slot(const uint64_t (&k)[5], uint32_t mask) {
  return (uint32_t)flow_hash64(k[0], k[1], k[2], k[3], k[4]) & mask;
}

__global__ __launch_bounds__(kPeerBlock) void k_peers_clear(uint32_t* table, uint32_t slots,
                                                            uint32_t* peer, uint32_t n_ids) {
  const uint32_t i = blockIdx.x * kPeerBlock + threadIdx.x;
  if (i < slots) table[i] = kNoPeer;
  if (i == 0) peer[n_ids] = kNoPeer;
}

// An entry is tcbee_flow_entry viewed as u64[8]: the tuple k0..k4, then the counts.
__global__ __launch_bounds__(kPeerBlock) void k_peers_insert(const uint64_t* ent, uint32_t n_ids,
                                                             uint32_t* table, uint32_t mask) {
  const uint32_t k = blockIdx.x * kPeerBlock + threadIdx.x;
  if (k >= n_ids) return;
  const uint64_t* e = ent + 8ull * k;
  const uint64_t key[5] = {e[0], e[1], e[2], e[3], e[4]};
  uint32_t slot = peer_slot(key, mask);
  for (uint32_t t = 0; t <= mask; ++t) {  // (at most half the slots are ever taken)
    if (atomicCAS(&table[slot], kNoPeer, k) == kNoPeer) return;
    slot = (slot + 1u) & mask;
  }
}

__global__ __launch_bounds__(kPeerBlock) void k_peers_probe(const uint64_t* ent, uint32_t n_ids,
                                                            const uint32_t* table, uint32_t mask,
                                                            uint32_t* peer) {
  const uint32_t k = blockIdx.x * kPeerBlock + threadIdx.x;
  if (k >= n_ids) return;
  const uint64_t* e = ent + 8ull * k;
  // src and dst addresses exchanged; k4 = sport | dport << 16 | protocol and padding << 32
  const uint64_t k4 = e[4];
  const uint64_t m[5] = {e[2], e[3], e[0], e[1],
                         (k4 & ~0xFFFFFFFFull) | ((k4 & 0xFFFFull) << 16) | ((k4 >> 16) & 0xFFFFull)};
  uint32_t slot = peer_slot(m, mask), found = kNoPeer;
  for (uint32_t t = 0; t <= mask; ++t) {
    const uint32_t id = table[slot];
    if (id == kNoPeer) break;
    if (id != k && id < n_ids) {
      const uint64_t* o = ent + 8ull * id;
      if (o[0] == m[0] && o[1] == m[1] && o[2] == m[2] && o[3] == m[3] && o[4] == m[4]) {
        found = id;
        break;
      }
    }
    slot = (slot + 1u) & mask;
  }
  peer[k] = found;
}

// ---------------------------------------------------------------------------
// The join
// ---------------------------------------------------------------------------
struct PeerArgs {
  tcbee_peer_in in;
  tcbee_peer_out out;
  uint32_t* q;    // [n_max]: rank of each record among its peer's
  int64_t* h;     // [n_max]: A after k_peer_rank, H after k_peer_scan
  uint8_t* hb;    // bit j: position j is the first of its segment
  uint64_t* agg;  // [tiles][2]: max, "holds a head"; a tile's carry-in after k_peer_carry
  uint32_t n_max, n_ids, lds;
};

__device__ __forceinline__ uint32_t peer_n(const PeerArgs& a) {
  return umin32(a.in.flow_start[a.n_ids + 1u], a.n_max);
}

// Segmented running maximum: m = max since the last head, f = "holds a head".
struct PMax {
  int64_t m;
  uint32_t f;
};
__device__ __forceinline__ PMax pmax_id() { return PMax{kNone, 0u}; }
__device__ __forceinline__ PMax combine(const PMax& l, const PMax& r) {
  if (r.f) return r;
  return PMax{l.m > r.m ? l.m : r.m, l.f};
}
__device__ __forceinline__ PMax shfl_up_v(const PMax& x, uint32_t o) {
  return PMax{(int64_t)__shfl_up((long long)x.m, o), __shfl_up(x.f, o)};
}
__device__ __forceinline__ void pmax_step(PMax& r, bool head, int64_t v) {
  if (head) r = PMax{v, 1u};
  else if (v > r.m) r.m = v;
}
__device__ __forceinline__ PMax agg_get(const uint64_t* p) {
  const pu64x2 v = *reinterpret_cast<const pu64x2*>(p);
  return PMax{(int64_t)v.x, (uint32_t)v.y};
}
__device__ __forceinline__ void agg_put(uint64_t* p, const PMax& r) {
  *reinterpret_cast<pu64x2*>(p) = pu64x2{(uint64_t)r.m, (uint64_t)r.f};
}

// What a run (the part of a segment inside one tile) adds to its stats row; every
// component combines exactly in any order.
struct PRun {
  uint64_t mn, mx, sum;
  int64_t out;
  uint32_t cnt, f;
};
__device__ __forceinline__ PRun prun_id() { return PRun{~0ull, 0ull, 0ull, kNone, 0u, 0u}; }
__device__ __forceinline__ PRun combine(const PRun& l, const PRun& r) {
  if (r.f) return r;
  return PRun{l.mn < r.mn ? l.mn : r.mn, l.mx > r.mx ? l.mx : r.mx, l.sum + r.sum,
              l.out > r.out ? l.out : r.out, l.cnt + r.cnt, l.f};
}
__device__ __forceinline__ PRun shfl_up_v(const PRun& x, uint32_t o) {
  return PRun{(uint64_t)__shfl_up((unsigned long long)x.mn, o),
              (uint64_t)__shfl_up((unsigned long long)x.mx, o),
              (uint64_t)__shfl_up((unsigned long long)x.sum, o),
              (int64_t)__shfl_up((long long)x.out, o), __shfl_up(x.cnt, o), __shfl_up(x.f, o)};
}

// A segment and its peer's, every bound clamped to n; c == d: no peer, or an empty one.
struct Seg {
  uint32_t k, a, b, c, d;
};
__device__ __forceinline__ Seg seg_load(const PeerArgs& A, uint32_t n, uint32_t k) {
  const uint32_t* fs = A.in.flow_start;
  Seg s;
  s.k = k;
  s.a = umin32(fs[k], n);
  s.b = umin32(fs[k + 1u], n);
  s.c = s.d = 0u;
  const uint32_t p = A.in.peer[k];
  if (p < A.n_ids) {
    s.c = umin32(fs[p], n);
    s.d = umax32(umin32(fs[p + 1u], n), s.c);
  }
  return s;
}

// first index in [lo, hi) with p[index] >= x, else hi
template <class T>
__device__ __forceinline__ uint32_t lower_bound(const T* p, uint32_t lo, uint32_t hi, T x) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (p[mid] < x) lo = mid + 1u;
    else hi = mid;
  }
  return lo;
}
// the same in [from, end), by doubling steps from `from` and then bisection: the cost
// follows the distance to the answer, not the length of the peer's segment
template <class T>
__device__ __forceinline__ uint32_t gallop(const T* p, uint32_t from, uint32_t end, T x) {
  uint32_t lo = from, hi = from, step = 1u;
  while (hi < end && p[hi] < x) {
    lo = hi + 1u;
    hi += step;
    step <<= 1;
  }
  return lower_bound(p, lo, umin32(hi, end), x);
}

template <class T>
__device__ __forceinline__ void peer_load8(const T* p, uint32_t g0, uint32_t n, T fill, T (&v)[8]) {
  if (g0 + kPeerItems <= n) {
    constexpr uint32_t per = 16 / sizeof(T);
    typedef T vec __attribute__((ext_vector_type(16 / sizeof(T))));
#pragma unroll
    for (uint32_t i = 0; i < kPeerItems; i += per) {
      const vec x = *reinterpret_cast<const vec*>(p + g0 + i);
#pragma unroll
      for (uint32_t e = 0; e < per; ++e) v[i + e] = x[e];
    }
  } else {
#pragma unroll
    for (uint32_t i = 0; i < kPeerItems; ++i) v[i] = g0 + i < n ? p[g0 + i] : fill;
  }
}
template <class T>
__device__ __forceinline__ void peer_store8(T* p, uint32_t g0, uint32_t valid, const T (&v)[8]) {
  if (valid == 0xFFu) {
    constexpr uint32_t per = 16 / sizeof(T);
    typedef T vec __attribute__((ext_vector_type(16 / sizeof(T))));
#pragma unroll
    for (uint32_t i = 0; i < kPeerItems; i += per) {
      vec x;
#pragma unroll
      for (uint32_t e = 0; e < per; ++e) x[e] = v[i + e];
      *reinterpret_cast<vec*>(p + g0 + i) = x;
    }
  } else {
#pragma unroll
    for (uint32_t i = 0; i < kPeerItems; ++i)
      if ((valid >> i) & 1u) p[g0 + i] = v[i];
  }
}

__device__ __forceinline__ uint32_t lane_valid(uint32_t g0, uint32_t n) {
  const uint32_t left = g0 < n ? n - g0 : 0u;
  return left >= kPeerItems ? 0xFFu : (1u << left) - 1u;
}

// Thread 0 places the tile: the segment of its first position, and whether the whole
// tile lies inside it while that segment's peer has records (`single`).
__device__ __forceinline__ void tile_place(const PeerArgs& A, uint32_t n, uint32_t tbase, Seg* s_seg,
                                           uint32_t* s_single) {
  const uint32_t last = umin32(tbase + kPeerTile, n) - 1u;
  const Seg s = seg_load(A, n, series_segment(A.in.flow_start, A.n_ids, tbase));
  *s_seg = s;
  *s_single = A.lds && last < s.b && s.d > s.c;
}

__global__ __launch_bounds__(kPeerBlock) void k_peer_rows(PeerArgs A) {
  const uint32_t k = blockIdx.x * kPeerBlock + threadIdx.x;
  if (k > A.n_ids) return;
  uint64_t* const row = reinterpret_cast<uint64_t*>(A.out.stats + k);
  row[0] = (uint64_t)A.in.peer[k];  // peer, rtt_samples
  row[1] = ~0ull;                   // rtt_min_ns
  row[2] = row[3] = 0ull;           // rtt_max_ns, rtt_sum_ns
  row[4] = (uint64_t)kNone;         // max_outstanding
}

// ---------------------------------------------------------------------------
// Rank: q and A of every position, the head bits, the tile's aggregate.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kPeerBlock) void k_peer_rank(PeerArgs A) {
  const uint32_t n = peer_n(A);
  const uint32_t tile = blockIdx.x, tbase = tile * kPeerTile;
  if (tbase >= n) return;
  __shared__ PMax s_w[kPeerWaves];
  __shared__ Seg s_seg;
  __shared__ uint32_t s_single, s_qlo;
  __shared__ uint32_t s_perm[kPeerLdsSlots];
  const uint32_t* const perm = A.in.perm;
  if (threadIdx.x == 0) {
    tile_place(A, n, tbase, &s_seg, &s_single);
    s_qlo = s_single ? lower_bound(perm + s_seg.c, 0u, s_seg.d - s_seg.c, perm[tbase]) : 0u;
  }
  __syncthreads();
  const bool single = s_single != 0u;
  const uint32_t qlo = s_qlo;
  Seg sg = s_seg;
  uint32_t slen = 0u;
  if (single) {  // the peer's perm from the tile's first rank on
    slen = umin32(kPeerLdsSlots, sg.d - sg.c - qlo);
    for (uint32_t t = threadIdx.x; t < slen; t += kPeerBlock) s_perm[t] = perm[sg.c + qlo + t];
    __syncthreads();
  }

  const uint32_t g0 = tbase + threadIdx.x * kPeerItems, valid = lane_valid(g0, n);
  uint32_t pm[kPeerItems], ak[kPeerItems], qv[kPeerItems];
  int64_t av[kPeerItems];
  peer_load8(perm, g0, n, 0u, pm);
  peer_load8(A.in.ack, g0, n, 0u, ak);
  if (!single && valid) sg = seg_load(A, n, series_segment(A.in.flow_start, A.n_ids, g0));
  uint32_t q = qlo, heads = 0u;
  bool first = !single;
  PMax r = pmax_id();
#pragma unroll
  for (uint32_t i = 0; i < kPeerItems; ++i) {
    qv[i] = 0u;
    av[i] = kNone;
    if (!((valid >> i) & 1u)) continue;
    const uint32_t j = g0 + i;
    if (!single) {
      while (j >= sg.b && sg.k < A.n_ids) {
        sg = seg_load(A, n, sg.k + 1u);
        q = 0u;
        first = true;
      }
    }
    const uint32_t len = sg.d - sg.c;
    if (len) {
      const uint32_t* const pp = perm + sg.c;
      const uint32_t x = pm[i];
      if (single) {
        if (qlo + slen == len || x <= s_perm[slen - 1u])
          q = qlo + lower_bound(s_perm, umin32(q - qlo, slen), slen, x);
        else
          q = gallop(pp, umax32(q, qlo + slen), len, x);
      } else {
        q = first ? lower_bound(pp, 0u, len, x) : gallop(pp, q, len, x);
        first = false;
      }
      if (q) {
        const uint32_t m = sg.c + q - 1u;  // the peer's latest record before j
        av[i] = A.in.seq_rel[m] + (int64_t)(int32_t)(ak[i] - A.in.seq[m]);
      }
      qv[i] = q;
    }
    const bool head = j == sg.a;
    heads |= (head ? 1u : 0u) << i;
    pmax_step(r, head, av[i]);
  }
  peer_store8(A.q, g0, valid, qv);
  peer_store8(A.h, g0, valid, av);
  if (valid) A.hb[g0 >> 3] = (uint8_t)heads;
  PMax total;
  (void)block_excl<kPeerWaves>(r, pmax_id(), s_w, total);
  if (threadIdx.x == 0) agg_put(A.agg + 2ull * tile, total);
}

// Carry: the aggregates of tiles [0, ceil(n / kPeerTile)) become their exclusive
// segmented scan, in place: agg[t] is the state at the end of tile t - 1.
__global__ __launch_bounds__(kPeerCarryBlock) void k_peer_carry(PeerArgs A) {
  const uint32_t n = peer_n(A);
  const uint32_t ntiles = (n + kPeerTile - 1u) / kPeerTile;
  __shared__ PMax s_w[kPeerCarryWaves];
  PMax carry = pmax_id();
  for (uint32_t t0 = 0; t0 < ntiles; t0 += kPeerCarryBlock * kPeerCarryItems) {
    const uint32_t t = t0 + threadIdx.x * kPeerCarryItems;
    PMax c[kPeerCarryItems], sum = pmax_id();
#pragma unroll
    for (uint32_t i = 0; i < kPeerCarryItems; ++i) {
      c[i] = t + i < ntiles ? agg_get(A.agg + 2ull * (t + i)) : pmax_id();
      sum = combine(sum, c[i]);
    }
    PMax total;
    PMax x = combine(carry, block_excl<kPeerCarryWaves>(sum, pmax_id(), s_w, total));
#pragma unroll
    for (uint32_t i = 0; i < kPeerCarryItems; ++i) {
      if (t + i < ntiles) agg_put(A.agg + 2ull * (t + i), x);
      x = combine(x, c[i]);
    }
    carry = combine(carry, total);
  }
}

// Scan: A -> H in place (a lane reads its eight positions before it writes them).
__global__ __launch_bounds__(kPeerBlock) void k_peer_scan(PeerArgs A) {
  const uint32_t n = peer_n(A);
  const uint32_t tile = blockIdx.x, tbase = tile * kPeerTile;
  if (tbase >= n) return;
  __shared__ PMax s_w[kPeerWaves];
  const uint32_t g0 = tbase + threadIdx.x * kPeerItems, valid = lane_valid(g0, n);
  int64_t v[kPeerItems];
  peer_load8<int64_t>(A.h, g0, n, kNone, v);
  const uint32_t heads = valid ? A.hb[g0 >> 3] & valid : 0u;
  PMax r = pmax_id();
#pragma unroll
  for (uint32_t i = 0; i < kPeerItems; ++i) pmax_step(r, (heads >> i) & 1u, v[i]);
  PMax unused;
  r = combine(agg_get(A.agg + 2ull * tile), block_excl<kPeerWaves>(r, pmax_id(), s_w, unused));
#pragma unroll
  for (uint32_t i = 0; i < kPeerItems; ++i) {
    pmax_step(r, (heads >> i) & 1u, v[i]);
    v[i] = r.m;
  }
  peer_store8(A.h, g0, valid, v);
}

// ---------------------------------------------------------------------------
// Apply. RTT: rtt_ns or stats is wanted (then ts_ns, mark, seq and seq_rel of the tile
// are read and the search for the acknowledging record runs).
// ---------------------------------------------------------------------------
template <bool RTT>
__global__ __launch_bounds__(kPeerBlock) void k_peer_apply(PeerArgs A) {
  const uint32_t n = peer_n(A);
  const uint32_t tile = blockIdx.x, tbase = tile * kPeerTile;
  if (tbase >= n) return;
  __shared__ PRun s_r[kPeerWaves];
  __shared__ Seg s_seg;
  __shared__ uint32_t s_single, s_qlo;
  __shared__ int64_t s_h[RTT ? kPeerLdsSlots : 1u];
  if (threadIdx.x == 0) {
    tile_place(A, n, tbase, &s_seg, &s_single);
    s_qlo = s_single ? umin32(A.q[tbase], s_seg.d - s_seg.c) : 0u;
  }
  __syncthreads();
  const bool single = s_single != 0u;
  const uint32_t qlo = s_qlo;
  Seg sg = s_seg;
  uint32_t slen = 0u;
  if (RTT && single) {  // the peer's H from the tile's first rank on
    slen = umin32(kPeerLdsSlots, sg.d - sg.c - qlo);
    for (uint32_t t = threadIdx.x; t < slen; t += kPeerBlock) s_h[t] = A.h[sg.c + qlo + t];
    __syncthreads();
  }

  const uint32_t g0 = tbase + threadIdx.x * kPeerItems, valid = lane_valid(g0, n);
  uint32_t qv[kPeerItems], sq[kPeerItems], mk[kPeerItems];
  int64_t sr[kPeerItems], una[kPeerItems], wnd[kPeerItems];
  uint64_t ts[kPeerItems], rtt[kPeerItems];
  uint32_t sq_next = 0u;
  peer_load8(A.q, g0, n, 0u, qv);
  if (RTT) {
    peer_load8(A.in.seq, g0, n, 0u, sq);
    peer_load8<int64_t>(A.in.seq_rel, g0, n, 0, sr);
    peer_load8<uint64_t>(A.in.ts_ns, g0, n, 0ull, ts);
    if (valid == 0xFFu) {
      const pu32x2 m = *reinterpret_cast<const pu32x2*>(A.in.mark + g0);
#pragma unroll
      for (uint32_t i = 0; i < kPeerItems; ++i) mk[i] = ((i < 4 ? m.x : m.y) >> (8u * (i & 3u))) & 0xFFu;
    } else {
#pragma unroll
      for (uint32_t i = 0; i < kPeerItems; ++i) mk[i] = (valid >> i) & 1u ? A.in.mark[g0 + i] : 0u;
    }
    if (g0 + kPeerItems < n) sq_next = A.in.seq[g0 + kPeerItems];
  }
  if (!single && valid) sg = seg_load(A, n, series_segment(A.in.flow_start, A.n_ids, g0));
  uint32_t heads = 0u, tails = 0u;
#pragma unroll
  for (uint32_t i = 0; i < kPeerItems; ++i) {
    una[i] = wnd[i] = kNone;
    rtt[i] = ~0ull;
    if (!((valid >> i) & 1u)) continue;
    const uint32_t j = g0 + i;
    if (!single) {
      while (j >= sg.b && sg.k < A.n_ids) sg = seg_load(A, n, sg.k + 1u);
    }
    heads |= (j == sg.a ? 1u : 0u) << i;
    tails |= (j + 1u == sg.b || j + 1u == n ? 1u : 0u) << i;
    const uint32_t len = sg.d - sg.c;
    const uint32_t q = umin32(qv[i], len);
    if (q) {
      const uint32_t m = sg.c + q - 1u;
      una[i] = A.h[m];
      if (A.out.wnd_edge && una[i] != kNone) wnd[i] = una[i] + (int64_t)A.in.window[m];
    }
    if (!RTT) continue;
    const int64_t s = sr[i];
    const uint32_t next = i + 1u < kPeerItems ? sq[(i + 1u) % kPeerItems] : sq_next;
    const bool elig = j + 1u < sg.b && (int32_t)(next - sq[i]) > 0 && !(mk[i] & 1u);
    if (elig && len && (una[i] == kNone || una[i] <= s)) {
      uint32_t f;  // first index of the peer's segment at or past q with H > s
      if (single) {
        const uint32_t st = q - qlo;
        if (st < slen && s_h[slen - 1u] > s) f = qlo + lower_bound(s_h, st, slen, s + 1);
        else if (qlo + slen == len) f = len;
        else f = gallop(A.h + sg.c, umax32(q, qlo + slen), len, s + 1);
      } else {
        f = gallop(A.h + sg.c, q, len, s + 1);
      }
      if (f < len) {
        const uint64_t tf = A.in.ts_ns[sg.c + f];
        rtt[i] = tf >= ts[i] ? tf - ts[i] : 0ull;
      }
    }
  }
  if (A.out.una) peer_store8(A.out.una, g0, valid, una);
  if (A.out.wnd_edge) peer_store8(A.out.wnd_edge, g0, valid, wnd);
  if (!RTT) return;
  if (A.out.rtt_ns) peer_store8(A.out.rtt_ns, g0, valid, rtt);
  if (!A.out.stats) return;

  // one set of atomics per run: a run ends with its segment and at the tile's end
  auto item = [&](uint32_t i) {
    if (!((valid >> i) & 1u)) return prun_id();
    const bool some = rtt[i] != ~0ull;
    return PRun{rtt[i], some ? rtt[i] : 0ull, some ? rtt[i] : 0ull,
                una[i] != kNone ? sr[i] - una[i] : kNone, some ? 1u : 0u, 0u};
  };
  PRun sum = prun_id();
#pragma unroll
  for (uint32_t i = 0; i < kPeerItems; ++i) {
    if ((heads >> i) & 1u) sum = PRun{~0ull, 0ull, 0ull, kNone, 0u, 1u};
    sum = combine(sum, item(i));
  }
  PRun total;
  PRun run = block_excl<kPeerWaves>(sum, prun_id(), s_r, total);
  if (threadIdx.x == kPeerBlock - 1u) tails |= valid & 0x80u;
  if (tails == 0u) return;
#pragma unroll
  for (uint32_t i = 0; i < kPeerItems; ++i) {
    if ((heads >> i) & 1u) run = prun_id();
    run = combine(run, item(i));
    if (!((tails >> i) & 1u)) continue;
    tcbee_peer_stats* const row =
        A.out.stats + (single ? s_seg.k : series_segment(A.in.flow_start, A.n_ids, g0 + i));
    if (run.cnt) {
      atomicAdd(&row->rtt_samples, run.cnt);
      atomicMin(reinterpret_cast<unsigned long long*>(&row->rtt_min_ns), (unsigned long long)run.mn);
      atomicMax(reinterpret_cast<unsigned long long*>(&row->rtt_max_ns), (unsigned long long)run.mx);
      atomicAdd(reinterpret_cast<unsigned long long*>(&row->rtt_sum_ns), (unsigned long long)run.sum);
    }
    if (run.out != kNone)
      (void)__hip_atomic_fetch_max(&row->max_outstanding, run.out, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {

constexpr uint64_t kPeerMaxRecords = 1ull << 31;  // n_max below it: u32 positions

bool peer_args_ok(uint64_t n_max, uint64_t n_ids) {
  return n_ids >= 1 && n_ids <= kMaxTableFlows && n_max < kPeerMaxRecords;
}

uint64_t peers_slots(uint64_t n_ids) {  // a power of two, at least 2 n_ids
  uint64_t s = 2;
  while (s < 2 * n_ids) s <<= 1;
  return s;
}

// Scratch of the join: q, then A / H, then the head bits, then 16 bytes per tile; every
// part a whole number of 16-byte vectors.
struct PeerLayout {
  uint64_t ntiles, h_off, hb_off, agg_off, bytes;
};
PeerLayout peer_layout(uint64_t n_max) {
  const uint64_t npad = (n_max + 31) & ~31ull;
  PeerLayout l;
  l.ntiles = (n_max + kPeerTile - 1) / kPeerTile;
  l.h_off = 4 * npad;
  l.hb_off = l.h_off + 8 * npad;
  l.agg_off = l.hb_off + ((npad / 8 + 15) & ~15ull);
  l.bytes = l.agg_off + 16 * (l.ntiles + 1);
  return l;
}

bool off_align(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace
}  // namespace tcbee

using namespace tcbee;

extern "C" {

static_assert(sizeof(tcbee_peer_stats) == 40, "tcbee_peer_stats is 40 bytes");
static_assert(sizeof(tcbee_flow_entry) == 64, "an entry is eight words");

uint64_t tcbee_peers_scratch_bytes(uint64_t n_ids) {
  if (n_ids < 1 || n_ids > kMaxTableFlows) return 0;
  return 4 * peers_slots(n_ids);
}

int tcbee_flow_peers_device(const tcbee_flow_entry* ent_dev, uint64_t n_ids, uint32_t* peer_dev,
                            void* scratch_dev, uint64_t scratch_bytes, void* stream) {
  if (!ent_dev || !peer_dev || !scratch_dev) return TCBEE_EINVAL;
  if (n_ids < 1 || n_ids > kMaxTableFlows) return TCBEE_EINVAL;
  if (off_align(ent_dev, 8) || off_align(peer_dev, 4) || off_align(scratch_dev, 4)) return TCBEE_EINVAL;
  if (scratch_bytes < tcbee_peers_scratch_bytes(n_ids)) return TCBEE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const uint32_t slots = (uint32_t)peers_slots(n_ids), ids = (uint32_t)n_ids;
  uint32_t* const table = static_cast<uint32_t*>(scratch_dev);
  const uint64_t* const ent = reinterpret_cast<const uint64_t*>(ent_dev);
  const unsigned gs = (slots + kPeerBlock - 1) / kPeerBlock, gi = (ids + kPeerBlock - 1) / kPeerBlock;
  hipLaunchKernelGGL(k_peers_clear, dim3(gs), dim3(kPeerBlock), 0, s, table, slots, peer_dev, ids);
  hipLaunchKernelGGL(k_peers_insert, dim3(gi), dim3(kPeerBlock), 0, s, ent, ids, table, slots - 1u);
  hipLaunchKernelGGL(k_peers_probe, dim3(gi), dim3(kPeerBlock), 0, s, ent, ids, table, slots - 1u,
                     peer_dev);
  return hipGetLastError() == hipSuccess ? TCBEE_OK : TCBEE_EDEVICE;
}

uint64_t tcbee_peer_scratch_bytes(uint64_t n_max, uint64_t n_ids) {
  if (!peer_args_ok(n_max, n_ids)) return 0;
  return peer_layout(n_max).bytes;
}

int tcbee_flow_peer_series_device(const tcbee_peer_in* in, uint64_t n_max, uint64_t n_ids,
                                  const tcbee_peer_out* out, void* scratch_dev,
                                  uint64_t scratch_bytes, void* stream) {
  if (!in || !out || !scratch_dev) return TCBEE_EINVAL;
  if (!in->flow_start || !in->peer || !in->perm || !in->seq || !in->ack || !in->seq_rel)
    return TCBEE_EINVAL;
  if (!out->una && !out->wnd_edge && !out->rtt_ns && !out->stats) return TCBEE_EINVAL;
  const bool rtt = out->rtt_ns || out->stats;
  if (out->wnd_edge && !in->window) return TCBEE_EINVAL;
  if (rtt && (!in->ts_ns || !in->mark)) return TCBEE_EINVAL;
  if (!peer_args_ok(n_max, n_ids)) return TCBEE_EINVAL;
  if (scratch_bytes < tcbee_peer_scratch_bytes(n_max, n_ids)) return TCBEE_EINVAL;
  if (off_align(in->perm, 16) || off_align(in->ts_ns, 16) || off_align(in->seq, 16) ||
      off_align(in->ack, 16) || off_align(in->window, 16) || off_align(in->seq_rel, 16) ||
      off_align(in->mark, 16) || off_align(out->una, 16) || off_align(out->wnd_edge, 16) ||
      off_align(out->rtt_ns, 16) || off_align(scratch_dev, 16))
    return TCBEE_EINVAL;
  if (off_align(in->flow_start, 4) || off_align(in->peer, 4) || off_align(out->stats, 8))
    return TCBEE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const PeerLayout l = peer_layout(n_max);
  uint8_t* const base = static_cast<uint8_t*>(scratch_dev);

  PeerArgs a{};
  a.in = *in;
  a.out = *out;
  a.q = reinterpret_cast<uint32_t*>(base);
  a.h = reinterpret_cast<int64_t*>(base + l.h_off);
  a.hb = base + l.hb_off;
  a.agg = reinterpret_cast<uint64_t*>(base + l.agg_off);
  a.n_max = (uint32_t)n_max;
  a.n_ids = (uint32_t)n_ids;
  a.lds = 1u;
#if TCBEE_VARIANTS
  // A/B hook (variants build only): every search in global memory, no staging
  if (const char* e = std::getenv("TCBEE_PEER_NOLDS")) a.lds = std::atoi(e) ? 0u : 1u;
#endif
  if (!out->wnd_edge) a.in.window = nullptr;
  if (!rtt) a.in.ts_ns = nullptr, a.in.mark = nullptr;

  if (out->stats) {
    const unsigned gr = (unsigned)((n_ids + 1 + kPeerBlock - 1) / kPeerBlock);
    hipLaunchKernelGGL(k_peer_rows, dim3(gr), dim3(kPeerBlock), 0, s, a);
  }
  const unsigned ntiles = (unsigned)l.ntiles;
  if (ntiles > 0) {
    hipLaunchKernelGGL(k_peer_rank, dim3(ntiles), dim3(kPeerBlock), 0, s, a);
    hipLaunchKernelGGL(k_peer_carry, dim3(1), dim3(kPeerCarryBlock), 0, s, a);
    hipLaunchKernelGGL(k_peer_scan, dim3(ntiles), dim3(kPeerBlock), 0, s, a);
    if (rtt) hipLaunchKernelGGL(k_peer_apply<true>, dim3(ntiles), dim3(kPeerBlock), 0, s, a);
    else hipLaunchKernelGGL(k_peer_apply<false>, dim3(ntiles), dim3(kPeerBlock), 0, s, a);
  }
  return hipGetLastError() == hipSuccess ? TCBEE_OK : TCBEE_EDEVICE;
}

}  // extern "C"
