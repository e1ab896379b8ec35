// Weighted Mann-Whitney counts of bootstrap replicates ([mi355x] auc_statistics): vv_auc_boot_counts of include/vecvad_hip.h.  All
// arithmetic is integer, every draw is a pure function of (seed, r, s, j) and no result depends on the order of anything: bit-identical
// run to run, whatever the launch.
//   Weights: W[r][i], one uint32 per replicate and frame, in the work buffer (zeroed first: a frame no video covers weighs nothing).
//     ab_block_weights (VV_AUC_UNIT_BLOCK), one workgroup per (replicate, video): the k block starts are drawn by the threads in turn
//       and entered into a difference array in LDS with integer atomics (4096 frames of the video at a time; a block is clipped to the
//       chunk, so no carry crosses a chunk), one scan in time order turns it into the weights.
//     ab_video_picks + ab_video_expand (VV_AUC_UNIT_VIDEO): one thread per (replicate, draw) counts its pick into the multiplicity table
//       mult[r][v] (integer atomics in global memory), one workgroup per (replicate, video) then copies the multiplicity to the frames.
//   Counts: ab_count_kernel, one workgroup per (replicate, group), walks the group's frames in score order, 1024 positions a tile.  With
//     Nx(p) / Px(p) the weighted negatives / positives in front of position p and head(p) the first position of p's tie group,
//       U2 = sum over positives w * Nx(head) + P * N - sum over negatives w * Px(head)
//     (a positive collects 2 per negative below and 1 per tied one; the two sums split that into "negatives in front of my tie group" and
//     "negatives up to the end of it", and the second is P * N less the mirrored sum over the negatives).  One scan per tile carries
//     (N, P, Nx(head), Px(head)) -- sums, and the values at the last head seen -- across threads, waves and tiles.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vecvad_hip.h"
#include "vv_common.h"

namespace {

typedef unsigned long long u64;

constexpr int AB_ITEMS = 4;                    // positions of a tile per thread, consecutive
constexpr int AB_TILE = VV_WG * AB_ITEMS;      // 1024
constexpr int AB_TL = 4096;                    // frames of a video per difference array
constexpr int AB_TPT = AB_TL / VV_WG;          // 16 entries of it per thread

__host__ __device__ inline u64 ab_mix(u64 x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// draw(seed, r, s, j, m) with h = mix(mix(mix(seed) ^ r) ^ s) taken once per (r, s); m < 2^32
__host__ __device__ inline uint32_t ab_draw(u64 h, u64 j, uint32_t m) { return (uint32_t)(((ab_mix(h ^ j) >> 32) * (u64)m) >> 32); }
__host__ __device__ inline u64 ab_key(u64 seed, u64 r, u64 s) { return ab_mix(ab_mix(ab_mix(seed) ^ r) ^ s); }

__device__ __forceinline__ int ab_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// exclusive sum of one int per thread over the workgroup; wtot: VV_WG / 64 ints of LDS.  Ends behind a barrier.
__device__ __forceinline__ int ab_excl_sum(const int v, int* wtot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int s = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(s, o);
    if (lane >= o) s += t;
  }
  __syncthreads();                             // wtot of the call before has been read
  if (lane == 63) wtot[wave] = s;
  __syncthreads();
  int base = 0;
  for (int k = 0; k < wave; ++k) base += wtot[k];
  return base + s - v;
}

__global__ void __launch_bounds__(VV_WG)
ab_block_weights(const int32_t* __restrict__ video_off, const int n, const int V, const u64 seed, const u64 r0, const int block,
                 uint32_t* __restrict__ W) {
  __shared__ int diff[AB_TL + 1];
  __shared__ int wtot[VV_WG / 64];
  const int tid = threadIdx.x;
  const int ri = blockIdx.x / V, v = blockIdx.x - ri * V;
  const int a = ab_clamp(video_off[v], n), e = ab_clamp(video_off[v + 1], n);
  const int L = e - a;
  if (L <= 0) return;
  const int b = block < L ? block : L;
  const int k = (L + b - 1) / b;
  const uint32_t m = (uint32_t)(L - b + 1);
  const u64 h = ab_key(seed, r0 + (u64)ri, (1ull << 32) + (u64)v);
  uint32_t* w = W + (int64_t)ri * n + a;
  for (int c0 = 0; c0 < L; c0 += AB_TL) {
    const int c1 = L - c0 < AB_TL ? L : c0 + AB_TL;
    for (int q = tid; q <= AB_TL; q += VV_WG) diff[q] = 0;
    __syncthreads();
    for (int j = tid; j < k; j += VV_WG) {
      const int s = (int)ab_draw(h, (u64)j, m);            // s + b <= L
      const int lo = s > c0 ? s : c0, hi = s + b < c1 ? s + b : c1;
      if (lo < hi) {
        atomicAdd(&diff[lo - c0], 1);
        atomicSub(&diff[hi - c0], 1);                      // hi - c0 <= AB_TL: the entry behind the chunk
      }
    }
    __syncthreads();
    int loc[AB_TPT];
    int s = 0;
#pragma unroll
    for (int q = 0; q < AB_TPT; ++q) {
      s += diff[tid * AB_TPT + q];
      loc[q] = s;
    }
    const int base = ab_excl_sum(s, wtot);                 // every thread has read its entries behind the barriers of the sum
#pragma unroll
    for (int q = 0; q < AB_TPT; ++q) diff[tid * AB_TPT + q] = base + loc[q];
    __syncthreads();
    for (int q = tid; q < c1 - c0; q += VV_WG) w[c0 + q] = (uint32_t)diff[q];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(VV_WG)
ab_video_picks(const int32_t* __restrict__ stratum_off, const int V, const int S, const int64_t total, const u64 seed, const u64 r0,
               uint32_t* __restrict__ mult) {
  const int64_t t = (int64_t)blockIdx.x * VV_WG + threadIdx.x;
  if (t >= total) return;
  const int ri = (int)(t / V), slot = (int)(t - (int64_t)ri * V);
  int lo = 0, hi = S;                          // the last stratum s with stratum_off[s] <= slot
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (stratum_off[mid] <= slot) lo = mid; else hi = mid;
  }
  const int s0 = stratum_off[lo], s1 = stratum_off[lo + 1];
  if (s0 < 0 || s1 > V || slot < s0 || slot >= s1) return;          // a table that is no CSR over the videos: memory stays protected
  const uint32_t pick = ab_draw(ab_key(seed, r0 + (u64)ri, (u64)lo), (u64)(slot - s0), (uint32_t)(s1 - s0));
  atomicAdd(&mult[(int64_t)ri * V + s0 + (int)pick], 1u);
}

__global__ void __launch_bounds__(VV_WG)
ab_video_expand(const int32_t* __restrict__ video_off, const int n, const int V, const uint32_t* __restrict__ mult,
                uint32_t* __restrict__ W) {
  const int ri = blockIdx.x / V, v = blockIdx.x - ri * V;
  const int a = ab_clamp(video_off[v], n), e = ab_clamp(video_off[v + 1], n);
  const uint32_t mv = mult[(int64_t)ri * V + v];
  uint32_t* w = W + (int64_t)ri * n;
  for (int i = a + threadIdx.x; i < e; i += VV_WG) w[i] = mv;
}

// what a run of positions adds up to: weighted negatives / positives, and -- when it holds the head of a tie group -- those in front of
// its last head, counted from the start of the run
struct AbState {
  u64 n, p, hn, hp;
  int has;
};
__device__ __forceinline__ AbState ab_join(const AbState& a, const AbState& b) {      // a, then b
  AbState r;
  r.n = a.n + b.n;
  r.p = a.p + b.p;
  r.has = a.has | b.has;
  r.hn = b.has ? a.n + b.hn : a.hn;
  r.hp = b.has ? a.p + b.hp : a.hp;
  return r;
}
__device__ __forceinline__ AbState ab_shfl_up(const AbState& s, const int o) {
  AbState r;
  r.n = __shfl_up(s.n, o);
  r.p = __shfl_up(s.p, o);
  r.hn = __shfl_up(s.hn, o);
  r.hp = __shfl_up(s.hp, o);
  r.has = __shfl_up(s.has, o);
  return r;
}

template <bool WEIGHTED>
__global__ void __launch_bounds__(VV_WG)
ab_count_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ tie, const uint8_t* __restrict__ label,
                const int32_t* __restrict__ group_off, const int n, const int G, const uint32_t* __restrict__ W,
                int64_t* __restrict__ out) {
  __shared__ AbState wstate[VV_WG / 64];
  __shared__ u64 wsum[2][VV_WG / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ri = blockIdx.x / G, g = blockIdx.x - ri * G;
  const int g0 = ab_clamp(group_off[g], n), g1 = ab_clamp(group_off[g + 1], n);
  const uint32_t* w = WEIGHTED ? W + (int64_t)ri * n : nullptr;
  AbState carry = {0, 0, 0, 0, 0};             // everything in front of the tile, absolute: the same in every thread
  u64 X = 0, Y = 0;
  for (int t0 = g0; t0 < g1; t0 += AB_TILE) {
    u64 wn[AB_ITEMS], wp[AB_ITEMS];
    bool head[AB_ITEMS];
    AbState mine = {0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < AB_ITEMS; ++k) {
      const int p = t0 + tid * AB_ITEMS + k;
      wn[k] = wp[k] = 0;
      head[k] = false;
      if (p < g1) {
        const int i = order[p];
        head[k] = p == g0 || tie[p] != tie[p - 1];
        if ((unsigned)i < (unsigned)n) {
          const u64 wi = WEIGHTED ? (u64)w[i] : 1ull;
          if (label[i]) wp[k] = wi; else wn[k] = wi;
        }
      }
      if (head[k]) {
        mine.has = 1;
        mine.hn = mine.n;
        mine.hp = mine.p;
      }
      mine.n += wn[k];
      mine.p += wp[k];
    }
    AbState inc = mine;                        // inclusive over the wave
    for (int o = 1; o < 64; o <<= 1) {
      const AbState t = ab_shfl_up(inc, o);
      if (lane >= o) inc = ab_join(t, inc);
    }
    __syncthreads();                           // wstate of the tile before has been read
    if (lane == 63) wstate[wave] = inc;
    __syncthreads();
    AbState front = carry;                     // everything in front of this thread
    for (int k = 0; k < wave; ++k) front = ab_join(front, wstate[k]);
    {
      AbState ex = ab_shfl_up(inc, 1);         // the wave in front of this lane
      if (lane > 0) front = ab_join(front, ex);
    }
    u64 rn = front.n, rp = front.p, hn = front.hn, hp = front.hp;
#pragma unroll
    for (int k = 0; k < AB_ITEMS; ++k) {
      if (head[k]) {
        hn = rn;
        hp = rp;
      }
      X += wp[k] * hn;
      Y += wn[k] * hp;
      rn += wn[k];
      rp += wp[k];
    }
    for (int k = 0; k < VV_WG / 64; ++k) carry = ab_join(carry, wstate[k]);
  }
  for (int o = 32; o > 0; o >>= 1) {
    X += __shfl_down(X, o);
    Y += __shfl_down(Y, o);
  }
  __syncthreads();
  if (lane == 0) {
    wsum[0][wave] = X;
    wsum[1][wave] = Y;
  }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < VV_WG / 64; ++k) {
      X += wsum[0][k];
      Y += wsum[1][k];
    }
    int64_t* o = out + ((int64_t)ri * G + g) * 3;
    o[0] = (int64_t)(X + carry.p * carry.n - Y);
    o[1] = (int64_t)carry.p;
    o[2] = (int64_t)carry.n;
  }
}

__host__ constexpr int64_t ab_align8(int64_t v) { return (v + 7) & ~(int64_t)7; }

bool ab_sizes_ok(int32_t n, int32_t V, int32_t R, int32_t unit) {
  return n >= 0 && V >= 0 && R >= 0 && (unit == VV_AUC_UNIT_NONE || unit == VV_AUC_UNIT_VIDEO || unit == VV_AUC_UNIT_BLOCK);
}

}  // namespace

// work: W uint32 [R][n] | mult uint32 [R][V] (VV_AUC_UNIT_VIDEO only), each padded to 8 bytes
extern "C" int64_t vv_auc_boot_work(int32_t n, int32_t V, int32_t R, int32_t unit) {
  if (!ab_sizes_ok(n, V, R, unit) || V > VV_AUC_BOOT_MAX_VIDEOS) return -1;
  if (unit == VV_AUC_UNIT_NONE) return 0;
  return ab_align8((int64_t)R * n * 4) + (unit == VV_AUC_UNIT_VIDEO ? ab_align8((int64_t)R * V * 4) : 0);
}

extern "C" int vv_auc_boot_counts(const int32_t* order, const int32_t* tie, const uint8_t* label, const int32_t* group_off,
                                  const int32_t* video_off, const int32_t* stratum_off, int32_t n, int32_t G, int32_t V, int32_t S,
                                  uint64_t seed, int64_t r0, int32_t R, int32_t unit, int32_t block, int64_t* out, void* work,
                                  vv_stream stream) {
  if (!ab_sizes_ok(n, V, R, unit) || G < 0 || S < 0 || r0 < 1 || block < 1) return VV_ERR_BAD_ARG;
  if (unit == VV_AUC_UNIT_NONE && R > 1) return VV_ERR_BAD_ARG;
  if (R == 0 || G == 0) return VV_OK;
  if (!out) return VV_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {                                // every group is empty
    const hipError_t e = hipMemsetAsync(out, 0, (size_t)R * G * 3 * sizeof(int64_t), st);
    return e != hipSuccess ? VV_HIP_STATUS(e) : VV_OK;
  }
  if (!order || !tie || !label || !group_off) return VV_ERR_BAD_ARG;
  if (V > VV_AUC_BOOT_MAX_VIDEOS || (int64_t)R * G > INT32_MAX || (int64_t)R * V > INT32_MAX) return VV_ERR_UNSUPPORTED;
  uint32_t* W = nullptr;
  if (unit != VV_AUC_UNIT_NONE) {
    if (!video_off || !work || ((uintptr_t)work & 7) || (unit == VV_AUC_UNIT_VIDEO && !stratum_off)) return VV_ERR_BAD_ARG;
    W = static_cast<uint32_t*>(work);
    const hipError_t e = hipMemsetAsync(work, 0, (size_t)vv_auc_boot_work(n, V, R, unit), st);
    if (e != hipSuccess) return VV_HIP_STATUS(e);
    if (unit == VV_AUC_UNIT_BLOCK && V > 0) {
      VV_LAUNCH(ab_block_weights, dim3((unsigned)(R * V)), dim3(VV_WG), 0, st, video_off, (int)n, (int)V, (u64)seed, (u64)r0, (int)block, W);
      VV_CHECK_LAUNCH();
    } else if (unit == VV_AUC_UNIT_VIDEO && V > 0 && S > 0) {
      uint32_t* mult = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(work) + ab_align8((int64_t)R * n * 4));
      const int64_t total = (int64_t)R * V;
      VV_LAUNCH(ab_video_picks, dim3((unsigned)((total + VV_WG - 1) / VV_WG)), dim3(VV_WG), 0, st, stratum_off, (int)V, (int)S, total,
                (u64)seed, (u64)r0, mult);
      VV_CHECK_LAUNCH();
      VV_LAUNCH(ab_video_expand, dim3((unsigned)(R * V)), dim3(VV_WG), 0, st, video_off, (int)n, (int)V, (const uint32_t*)mult, W);
      VV_CHECK_LAUNCH();
    }
    VV_LAUNCH(ab_count_kernel<true>, dim3((unsigned)(R * G)), dim3(VV_WG), 0, st, order, tie, label, group_off, (int)n, (int)G,
              (const uint32_t*)W, out);
  } else {
    VV_LAUNCH(ab_count_kernel<false>, dim3((unsigned)(R * G)), dim3(VV_WG), 0, st, order, tie, label, group_off, (int)n, (int)G,
              (const uint32_t*)nullptr, out);
  }
  VV_CHECK_LAUNCH();
  return VV_OK;
}
