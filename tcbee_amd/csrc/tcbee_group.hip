// tcbee_group.hip — regroup a batch's records by flow on the device (DESIGN.md
// "Grouping by flow"): a stable LSD radix sort of (key, input index) pairs, the
// per-flow bounds, and the gather of the per-flow series as columns. Context-free:
// the caller owns every buffer, nothing is allocated and nothing synchronises in
// the device call, and no kernel waits on another workgroup — order between the
// steps comes from the launches on the stream alone.
//
// Per sort pass (P = ceil(B / 8) passes of ceil(B / P) bits, B = bit_length(n_ids)):
//   k_group_hist     per tile of kGroupTile records: digit counts, hist[digit][tile]
//   k_group_scan     one workgroup per digit: exclusive scan of its row, row total
//   k_group_scatter  per tile: stable rank in LDS, digit runs leave coalesced
// then k_group_bounds (flow_start = lower bounds in the sorted keys) and
// k_group_gather (columns of record perm[j] at grouped position j).
#include "tcbee_table.h"

namespace tcbee {

constexpr uint32_t kGroupBlock = 256;
constexpr uint32_t kGroupWaves = kGroupBlock / 64;
constexpr uint32_t kGroupTile = 4096;                      // records per workgroup
constexpr uint32_t kGroupItems = kGroupTile / kGroupBlock;  // records per lane
constexpr uint32_t kGroupRun = kGroupTile / kGroupWaves;    // records per wave
constexpr uint32_t kGroupRadixMax = 256;                    // 8 bits per pass at most
static_assert(kGroupRadixMax <= kGroupBlock, "one thread per digit in the tile scans");
static_assert(kGroupItems % 4 == 0, "k_group_hist loads 16-byte vectors");

struct GroupPass {
  const uint32_t* in_key;   // pass 0: the caller's flow ids (index implicit)
  const uint32_t* in_idx;
  uint32_t* out_key;
  uint32_t* out_idx;        // last pass: out->perm when the caller wants it
  uint32_t* hist;           // [radix][ntiles_max], digit-major
  uint32_t* rowtot;         // [radix] records per digit
  const uint64_t* n_dev;
  uint32_t n_max;
  uint32_t n_ids;
  uint32_t ntiles_max;      // row stride of hist
  uint32_t shift, bits;     // this pass's digit = (key >> shift) & ((1 << bits) - 1)
};

struct GroupGather {
  const uint8_t* rec;
  uint64_t rec_bytes;       // 74 * n_max: no byte at or past it is read
  const uint32_t* perm;
  const uint64_t* n_dev;
  uint32_t n_max;
  tcbee_group_out out;
};

__device__ __forceinline__ uint32_t group_n(const uint64_t* n_dev, uint32_t n_max) {
  if (n_dev == nullptr) return n_max;
  const uint64_t n = *n_dev;
  return n < n_max ? (uint32_t)n : n_max;
}

// Lanes of the wave whose item is valid and has this lane's digit: one ballot per
// digit bit (0 for a lane whose own item is not valid).
__device__ __forceinline__ uint64_t digit_peers(uint32_t d, bool valid, uint32_t bits) {
  uint64_t peers = __ballot(valid);
  for (uint32_t b = 0; b < bits; ++b) {
    const bool one = (d >> b) & 1u;
    const uint64_t bal = __ballot(one);
    peers &= one ? bal : ~bal;
  }
  return valid ? peers : 0ull;
}

// (block_excl_scan: tcbee_table.h, one value per thread of a 256-thread workgroup)
static_assert(kGroupBlock == 256, "block_excl_scan scans four waves");

// ---------------------------------------------------------------------------
// Histogram: digit counts of one tile. Counting needs no order, so a lane takes four
// 16-byte vectors of consecutive keys; a wave adds once per distinct digit.
// ---------------------------------------------------------------------------
template <bool FIRST>
__global__ __launch_bounds__(kGroupBlock) void k_group_hist(GroupPass a) {
  const uint32_t n = group_n(a.n_dev, a.n_max);
  const uint32_t tile = blockIdx.x, tbase = tile * kGroupTile;
  if (tbase >= n) return;
  const uint32_t ntile = n - tbase < kGroupTile ? n - tbase : kGroupTile;
  __shared__ uint32_t s_hist[kGroupRadixMax];
  const uint32_t tid = threadIdx.x, radix = 1u << a.bits, mask = radix - 1u;
  s_hist[tid] = 0u;
  // pass 0 reads the caller's ids: any 4-byte alignment, and no word past n_max
  const bool vec_ok = !FIRST || (reinterpret_cast<uintptr_t>(a.in_key) & 15u) == 0;
  uint32_t key[kGroupItems];
#pragma unroll
  for (uint32_t v = 0; v < kGroupItems / 4; ++v) {
    const uint32_t r = (v * kGroupBlock + tid) * 4u;  // first of four records, tile-local
    if (vec_ok && r + 4u <= ntile) {
      const u32x4 q = *reinterpret_cast<const u32x4*>(a.in_key + tbase + r);
      key[4 * v + 0] = q.x; key[4 * v + 1] = q.y; key[4 * v + 2] = q.z; key[4 * v + 3] = q.w;
    } else {
#pragma unroll
      for (uint32_t c = 0; c < 4; ++c) key[4 * v + c] = r + c < ntile ? a.in_key[tbase + r + c] : 0u;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t u = 0; u < kGroupItems; ++u) {
    const uint32_t r = ((u >> 2) * kGroupBlock + tid) * 4u + (u & 3u);
    const bool valid = r < ntile;
    const uint32_t k = FIRST ? (key[u] < a.n_ids ? key[u] : a.n_ids) : key[u];
    const uint32_t d = (k >> a.shift) & mask;
    const uint32_t d0 = __builtin_amdgcn_readfirstlane(d);
    if (__all(valid && d == d0)) {  // the hot-flow case: one add for the wave
      if (__lane_id() == 0) atomicAdd(&s_hist[d0], 64u);
    } else {
      const uint64_t peers = digit_peers(d, valid, a.bits);
      if (valid && (peers & lanemask_lt()) == 0) atomicAdd(&s_hist[d], (uint32_t)__popcll(peers));
    }
  }
  __syncthreads();
  if (tid < radix) a.hist[(uint64_t)tid * a.ntiles_max + tile] = s_hist[tid];
}

// ---------------------------------------------------------------------------
// Scan: workgroup d turns row d of the histogram (tiles [0, ceil(n / tile))) into its
// exclusive prefix, in place, and leaves the row's total. Rows are independent; the
// scatter adds the totals of the lower digits itself.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kGroupBlock) void k_group_scan(GroupPass a) {
  const uint32_t n = group_n(a.n_dev, a.n_max);
  const uint32_t ntiles = (n + kGroupTile - 1) / kGroupTile;
  __shared__ uint32_t s_w[kGroupWaves];
  uint32_t* const row = a.hist + (uint64_t)blockIdx.x * a.ntiles_max;
  uint32_t carry = 0;
  for (uint32_t t0 = 0; t0 < ntiles; t0 += 4u * kGroupBlock) {
    const uint32_t t = t0 + 4u * threadIdx.x;
    uint32_t c[4], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      c[j] = t + j < ntiles ? row[t + j] : 0u;
      sum += c[j];
    }
    uint32_t total;
    uint32_t x = carry + block_excl_scan(sum, s_w, total);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      if (t + j < ntiles) row[t + j] = x;
      x += c[j];
    }
    carry += total;
  }
  if (threadIdx.x == 0) a.rowtot[blockIdx.x] = carry;
}

// ---------------------------------------------------------------------------
// Scatter: the tile again, ranked stably. Wave w owns records [w * kGroupRun, +kGroupRun)
// of the tile and item u of lane l is record u * 64 + l of that run, so a record's
// rank among the tile's equal digits is
//   (equal digits in earlier waves) + (in this wave's earlier items) + (in lower lanes
//   of this item),
// the first from the per-wave counters once every wave has counted, the second from
// the wave's counter as it stood before item u (fetched by the add of the item's
// lowest peer lane and passed to the peers), the third from the ballots.
// ---------------------------------------------------------------------------
template <bool FIRST>
__global__ __launch_bounds__(kGroupBlock) void k_group_scatter(GroupPass a) {
  const uint32_t n = group_n(a.n_dev, a.n_max);
  const uint32_t tile = blockIdx.x, tbase = tile * kGroupTile;
  if (tbase >= n) return;
  const uint32_t ntile = n - tbase < kGroupTile ? n - tbase : kGroupTile;
  __shared__ uint32_t s_key[kGroupTile], s_idx[kGroupTile];
  __shared__ uint32_t s_cnt[kGroupWaves][kGroupRadixMax];
  __shared__ uint32_t s_start[kGroupRadixMax], s_gbase[kGroupRadixMax], s_w[kGroupWaves];
  const uint32_t tid = threadIdx.x, lane = __lane_id(), wave = tid >> 6;
  const uint32_t radix = 1u << a.bits, mask = radix - 1u;
#pragma unroll
  for (uint32_t w = 0; w < kGroupWaves; ++w) s_cnt[w][tid] = 0u;

  // every load of the lane is issued before the first use; a lane past the tile's end
  // re-reads the tile's first record (never used)
  uint32_t key[kGroupItems], idx[kGroupItems];
#pragma unroll
  for (uint32_t u = 0; u < kGroupItems; ++u) {
    const uint32_t r = wave * kGroupRun + u * 64u + lane;
    const uint32_t g = tbase + (r < ntile ? r : 0u);
    key[u] = __builtin_nontemporal_load(a.in_key + g);
    if (!FIRST) idx[u] = __builtin_nontemporal_load(a.in_idx + g);
  }
  if (FIRST) {
#pragma unroll
    for (uint32_t u = 0; u < kGroupItems; ++u) {
      key[u] = key[u] < a.n_ids ? key[u] : a.n_ids;
      idx[u] = tbase + wave * kGroupRun + u * 64u + lane;
    }
  }
  __syncthreads();

  uint32_t loc[kGroupItems];  // rank among the wave's equal digits
#pragma unroll
  for (uint32_t u = 0; u < kGroupItems; ++u) {
    const bool valid = wave * kGroupRun + u * 64u + lane < ntile;
    const uint32_t d = (key[u] >> a.shift) & mask;
    const uint32_t d0 = __builtin_amdgcn_readfirstlane(d);
    if (__all(valid && d == d0)) {  // 64 records of one digit: rank = lane
      uint32_t pre = 0;
      if (lane == 0) pre = atomicAdd(&s_cnt[wave][d0], 64u);
      loc[u] = __builtin_amdgcn_readfirstlane(pre) + lane;
    } else {
      const uint64_t peers = digit_peers(d, valid, a.bits);
      const uint32_t below = (uint32_t)__popcll(peers & lanemask_lt());
      uint32_t pre = 0;
      if (valid && below == 0) pre = atomicAdd(&s_cnt[wave][d], (uint32_t)__popcll(peers));
      const int leader = valid ? __ffsll((unsigned long long)peers) - 1 : (int)lane;
      loc[u] = __shfl(pre, leader) + below;
    }
  }
  __syncthreads();

  // thread d: the tile's records of digit d, where they start in the sorted tile, and
  // the global base of that run
  {
    uint32_t tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < kGroupWaves; ++w) {
      const uint32_t c = s_cnt[w][tid];
      s_cnt[w][tid] = tot;  // now: equal digits in earlier waves
      tot += c;
    }
    uint32_t unused;
    const uint32_t tstart = block_excl_scan(tot, s_w, unused);
    const uint32_t dbase = block_excl_scan(tid < radix ? a.rowtot[tid] : 0u, s_w, unused);
    const uint32_t tpre = tid < radix ? a.hist[(uint64_t)tid * a.ntiles_max + tile] : 0u;
    s_start[tid] = tstart;
    s_gbase[tid] = dbase + tpre - tstart;  // destination of sorted position p: s_gbase + p
  }
  __syncthreads();
#pragma unroll
  for (uint32_t u = 0; u < kGroupItems; ++u) {
    const bool valid = wave * kGroupRun + u * 64u + lane < ntile;
    const uint32_t d = (key[u] >> a.shift) & mask;
    const uint32_t pos = s_start[d] + s_cnt[wave][d] + loc[u];
    if (valid && pos < kGroupTile) {
      s_key[pos] = key[u];
      s_idx[pos] = idx[u];
    }
  }
  __syncthreads();
  // consecutive lanes take consecutive sorted positions: each digit run of the tile
  // is stored as one contiguous run
#pragma unroll
  for (uint32_t j = 0; j < kGroupItems; ++j) {
    const uint32_t pos = j * kGroupBlock + tid;
    if (pos < ntile) {
      const uint32_t k = s_key[pos];
      const uint32_t dst = s_gbase[(k >> a.shift) & mask] + pos;
      if (dst < n) {
        a.out_key[dst] = k;
        a.out_idx[dst] = s_idx[pos];
      }
    }
  }
}

// flow_start[k] = records with key < k = lower bound of k in the sorted keys
__global__ __launch_bounds__(kGroupBlock) void k_group_bounds(const uint32_t* keys,
                                                              const uint64_t* n_dev, uint32_t n_max,
                                                              uint32_t n_ids, uint32_t* flow_start) {
  const uint32_t n = group_n(n_dev, n_max);
  const uint32_t k = blockIdx.x * kGroupBlock + threadIdx.x;
  if (k > n_ids + 1u) return;
  uint32_t lo = 0, len = n;
  while (len > 0) {
    const uint32_t half = len >> 1, mid = lo + half;
    if (keys[mid] < k) {
      lo = mid + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  flow_start[k] = lo;
}

// ---------------------------------------------------------------------------
// Series gather: lane j reads record perm[j] (2-byte aligned: 74 i) through the
// 16-byte aligned chunks that hold its bytes [0, 8) and [52, 70), bounds-checked
// against the buffer's end, and stores the requested columns at j.
// ---------------------------------------------------------------------------
// 16 bytes at rec[a, a + 16), zero at and past `end` (a is 16-byte aligned)
__device__ __forceinline__ void group_chunk(const uint8_t* rec, uint64_t end, uint64_t a,
                                            uint32_t* c) {
  if (a + 16 <= end) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(rec + a);
    c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
    return;
  }
  c[0] = c[1] = c[2] = c[3] = 0u;
#pragma unroll
  for (uint32_t b = 0; b < 16; ++b)
    if (a + b < end) c[b >> 2] |= (uint32_t)rec[a + b] << (8 * (b & 3));
}

// out = bytes [o, o + 4 NDW) of the dwords c (o < 16): a dword shift by two select
// stages and a byte align, fetch_bytes' normalisation (tcbee_kernels.hip)
template <int NDW, int NC>
__device__ __forceinline__ void take_bytes(const uint32_t (&c)[NC], uint32_t o, uint32_t (&out)[NDW]) {
  static_assert(NC >= NDW + 4, "the select stages read c[NDW + 3]");
  const uint32_t q = o >> 2, r = o & 3u;
  const uint32_t m1 = 0u - (q & 1u), m2 = 0u - ((q >> 1) & 1u);
  uint32_t t[NDW + 3];
#pragma unroll
  for (int j = 0; j < NDW + 3; ++j) t[j] = (c[j] & ~m1) | (c[j + 1] & m1);
  uint32_t v2[NDW + 1];
#pragma unroll
  for (int j = 0; j < NDW + 1; ++j) v2[j] = (t[j] & ~m2) | (t[j + 2] & m2);
#pragma unroll
  for (int j = 0; j < NDW; ++j) out[j] = align_bytes(v2[j + 1], v2[j], r);
}

// TS: the time column is wanted (record bytes [0, 8)); TCP: any of seq .. flags is
// (bytes [52, 70)). A column that is not wanted costs neither its loads nor its store.
template <bool TS, bool TCP>
__global__ __launch_bounds__(kGroupBlock) void k_group_gather(GroupGather g) {
  const uint32_t n = group_n(g.n_dev, g.n_max);
  const uint32_t j = blockIdx.x * kGroupBlock + threadIdx.x;
  if (j >= n) return;
  const uint32_t i = g.perm[j];
  if (i >= g.n_max) return;  // (never for a permutation of [0, n))
  const uint64_t a = (uint64_t)kRecBytes * i;
  uint32_t c1[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  uint32_t c2[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  const uint32_t o1 = (uint32_t)(a & 15u), o2 = (uint32_t)((a + kRecSeq) & 15u);
  if (TS) {
    group_chunk(g.rec, g.rec_bytes, a & ~15ull, c1);
    if (o1 > 8u) group_chunk(g.rec, g.rec_bytes, (a & ~15ull) + 16, c1 + 4);
  }
  if (TCP) {  // 18 bytes from offset o2 <= 14: always two chunks
    const uint64_t b = (a + kRecSeq) & ~15ull;
    group_chunk(g.rec, g.rec_bytes, b, c2);
    group_chunk(g.rec, g.rec_bytes, b + 16, c2 + 4);
  }
  if (TS) {
    uint32_t t[2];
    take_bytes(c1, o1, t);
    g.out.ts_ns[j] = (uint64_t)t[0] | ((uint64_t)t[1] << 32);
  }
  if (TCP) {
    uint32_t f[5];  // record bytes [52, 72)
    take_bytes(c2, o2, f);
    if (g.out.seq) g.out.seq[j] = f[0];
    if (g.out.ack) g.out.ack[j] = f[1];
    if (g.out.window) g.out.window[j] = (uint16_t)(f[2] & 0xFFFFu);
    if (g.out.checksum) g.out.checksum[j] = (uint16_t)(f[4] & 0xFFFFu);
    if (g.out.flags) {
      // bytes 62..67 = urg, ack, psh, rst, syn, fin -> bits 5..0
      const uint32_t fl = ((f[2] & 0x00FF0000u) ? 32u : 0u) | ((f[2] & 0xFF000000u) ? 16u : 0u) |
                          ((f[3] & 0x000000FFu) ? 8u : 0u) | ((f[3] & 0x0000FF00u) ? 4u : 0u) |
                          ((f[3] & 0x00FF0000u) ? 2u : 0u) | ((f[3] & 0xFF000000u) ? 1u : 0u);
      g.out.flags[j] = (uint8_t)fl;
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {

int group_err(hipError_t e) {
  if (e == hipSuccess) return TCBEE_OK;
  if (e == hipErrorOutOfMemory) return TCBEE_ENOMEM;
  if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return TCBEE_ENODEV;
  return TCBEE_EDEVICE;
}
#define TRY_HIP(expr)                            \
  do {                                           \
    hipError_t e_ = (expr);                      \
    if (e_ != hipSuccess) return group_err(e_);  \
  } while (0)

constexpr uint64_t kGroupMaxRecords = 1ull << 31;  // n_max below it: u32 positions

// Scratch, in u32 words: two ping-pong (key, index) pairs of n_max rounded up to 4 (every
// array 16-byte aligned), the histogram at the widest radix (so the size does not
// depend on how n_ids splits into passes), the row totals.
struct GroupLayout {
  uint64_t n_pad, ntiles, words;
  uint64_t key(int b) const { return (uint64_t)b * 2 * n_pad; }
  uint64_t idx(int b) const { return (uint64_t)b * 2 * n_pad + n_pad; }
  uint64_t hist() const { return 4 * n_pad; }
  uint64_t rowtot() const { return 4 * n_pad + ntiles * kGroupRadixMax; }
};
GroupLayout group_layout(uint64_t n_max) {
  GroupLayout l;
  l.n_pad = (n_max + 3) & ~3ull;
  l.ntiles = (n_max + kGroupTile - 1) / kGroupTile;
  l.words = 4 * l.n_pad + l.ntiles * kGroupRadixMax + kGroupRadixMax;
  return l;
}

bool group_args_ok(uint64_t n_max, uint64_t n_ids) {
  return n_ids >= 1 && n_ids <= kMaxTableFlows && n_max < kGroupMaxRecords;
}

}  // namespace
}  // namespace tcbee

using namespace tcbee;

extern "C" {

uint64_t tcbee_group_scratch_bytes(uint64_t n_max, uint64_t n_ids) {
  if (!group_args_ok(n_max, n_ids)) return 0;
  return group_layout(n_max).words * sizeof(uint32_t);
}

int tcbee_group_by_flow_device(const uint8_t* rec74_dev, const uint32_t* flow_id_dev,
                               const uint64_t* n_dev, uint64_t n_max, uint64_t n_ids,
                               const tcbee_group_out* out, void* scratch_dev,
                               uint64_t scratch_bytes, void* stream) {
  if (!rec74_dev || !flow_id_dev || !out || !out->flow_start || !scratch_dev) return TCBEE_EINVAL;
  if (!group_args_ok(n_max, n_ids)) return TCBEE_EINVAL;
  if (scratch_bytes < tcbee_group_scratch_bytes(n_max, n_ids)) return TCBEE_EINVAL;
  if ((reinterpret_cast<uintptr_t>(rec74_dev) & 15u) || (reinterpret_cast<uintptr_t>(scratch_dev) & 15u))
    return TCBEE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const GroupLayout l = group_layout(n_max);
  uint32_t* const w = static_cast<uint32_t*>(scratch_dev);

  uint32_t B = 0;  // bit_length(n_ids): the keys are 0 .. n_ids
  while (B < 32 && (n_ids >> B) != 0) ++B;
  const uint32_t P = (B + 7) / 8, bits = (B + P - 1) / P;
  const bool columns = out->ts_ns || out->seq || out->ack || out->window || out->checksum || out->flags;
  // the gather reads the permutation: in out->perm, or in scratch when that is NULL
  uint32_t* const perm = out->perm ? out->perm : w + l.idx((P - 1) & 1);
  const unsigned ntiles = (unsigned)l.ntiles;

  GroupPass a{};
  a.hist = w + l.hist();
  a.rowtot = w + l.rowtot();
  a.n_dev = n_dev;
  a.n_max = (uint32_t)n_max;
  a.n_ids = (uint32_t)n_ids;
  a.ntiles_max = ntiles;
  a.bits = bits;
  for (uint32_t p = 0; p < P && ntiles > 0; ++p) {
    a.in_key = p == 0 ? flow_id_dev : w + l.key((p - 1) & 1);
    a.in_idx = p == 0 ? nullptr : w + l.idx((p - 1) & 1);
    a.out_key = w + l.key(p & 1);
    a.out_idx = p == P - 1 ? perm : w + l.idx(p & 1);
    a.shift = p * bits;
    if (p == 0) {
      hipLaunchKernelGGL(k_group_hist<true>, dim3(ntiles), dim3(kGroupBlock), 0, s, a);
    } else {
      hipLaunchKernelGGL(k_group_hist<false>, dim3(ntiles), dim3(kGroupBlock), 0, s, a);
    }
    hipLaunchKernelGGL(k_group_scan, dim3(1u << bits), dim3(kGroupBlock), 0, s, a);
    if (p == 0) {
      hipLaunchKernelGGL(k_group_scatter<true>, dim3(ntiles), dim3(kGroupBlock), 0, s, a);
    } else {
      hipLaunchKernelGGL(k_group_scatter<false>, dim3(ntiles), dim3(kGroupBlock), 0, s, a);
    }
    TRY_HIP(hipGetLastError());
  }
  const unsigned gb = (unsigned)((n_ids + 2 + kGroupBlock - 1) / kGroupBlock);
  hipLaunchKernelGGL(k_group_bounds, dim3(gb), dim3(kGroupBlock), 0, s, w + l.key((P - 1) & 1), n_dev,
                     (uint32_t)n_max, (uint32_t)n_ids, out->flow_start);
  if (columns && n_max > 0) {
    GroupGather g{};
    g.rec = rec74_dev;
    g.rec_bytes = (uint64_t)kRecBytes * n_max;
    g.perm = perm;
    g.n_dev = n_dev;
    g.n_max = (uint32_t)n_max;
    g.out = *out;
    const unsigned gg = (unsigned)((n_max + kGroupBlock - 1) / kGroupBlock);
    const bool tcp = out->seq || out->ack || out->window || out->checksum || out->flags;
    if (out->ts_ns && tcp) {
      hipLaunchKernelGGL((k_group_gather<true, true>), dim3(gg), dim3(kGroupBlock), 0, s, g);
    } else if (tcp) {
      hipLaunchKernelGGL((k_group_gather<false, true>), dim3(gg), dim3(kGroupBlock), 0, s, g);
    } else {
      hipLaunchKernelGGL((k_group_gather<true, false>), dim3(gg), dim3(kGroupBlock), 0, s, g);
    }
  }
  TRY_HIP(hipGetLastError());
  return TCBEE_OK;
}

int tcbee_group_by_flow(int device, const uint8_t* rec74, const uint32_t* flow_id, uint64_t n,
                        uint64_t n_ids, const tcbee_group_out* out_host) {
  if (!out_host || !out_host->flow_start || (n && (!rec74 || !flow_id))) return TCBEE_EINVAL;
  if (!group_args_ok(n, n_ids)) return TCBEE_EINVAL;
  TRY_HIP(hipSetDevice(device));
  // one allocation, cut into 16-byte aligned parts: records, ids, scratch, outputs
  const uint64_t width[8] = {4, 4, 8, 4, 4, 2, 2, 1};
  const uint64_t count[8] = {n_ids + 2, n, n, n, n, n, n, n};
  void* const host[8] = {out_host->flow_start, out_host->perm, out_host->ts_ns, out_host->seq,
                         out_host->ack, out_host->window, out_host->checksum, out_host->flags};
  auto pad = [](uint64_t b) { return (b + 15) & ~15ull; };
  const uint64_t rec_b = pad(kRecBytes * n + 16), id_b = pad(4 * n + 16);
  const uint64_t scr_b = pad(tcbee_group_scratch_bytes(n, n_ids));
  uint64_t off[8], total = rec_b + id_b + scr_b;
  for (int k = 0; k < 8; ++k) {
    off[k] = total;
    if (host[k]) total += pad(width[k] * count[k] + 16);
  }
  uint8_t* d = nullptr;
  TRY_HIP(hipMalloc(reinterpret_cast<void**>(&d), total));
  hipStream_t s = nullptr;
  int rc = TCBEE_OK;
  auto step = [&](hipError_t e) {
    if (rc == TCBEE_OK) rc = group_err(e);
    return rc == TCBEE_OK;
  };
  if (step(hipStreamCreateWithFlags(&s, hipStreamNonBlocking))) {
    if (n) {
      step(hipMemcpyAsync(d, rec74, kRecBytes * n, hipMemcpyHostToDevice, s));
      step(hipMemcpyAsync(d + rec_b, flow_id, 4 * n, hipMemcpyHostToDevice, s));
    }
    tcbee_group_out o{};
    void** const dev[8] = {(void**)&o.flow_start, (void**)&o.perm, (void**)&o.ts_ns, (void**)&o.seq,
                           (void**)&o.ack, (void**)&o.window, (void**)&o.checksum, (void**)&o.flags};
    for (int k = 0; k < 8; ++k) *dev[k] = host[k] ? d + off[k] : nullptr;
    if (rc == TCBEE_OK)
      rc = tcbee_group_by_flow_device(d, reinterpret_cast<const uint32_t*>(d + rec_b), nullptr, n,
                                      n_ids, &o, d + rec_b + id_b, scr_b, s);
    for (int k = 0; k < 8 && rc == TCBEE_OK; ++k)
      if (host[k] && count[k])
        step(hipMemcpyAsync(host[k], *dev[k], width[k] * count[k], hipMemcpyDeviceToHost, s));
    // (also after an error: nothing of this call is left running when d is freed)
    const hipError_t e = hipStreamSynchronize(s);
    step(e);
    (void)hipStreamDestroy(s);
  }
  (void)hipFree(d);
  return rc;
}

}  // extern "C"
