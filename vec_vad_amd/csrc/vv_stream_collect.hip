// Training from pushed frames (vec_vad_amd/stream_train.py): vv_stream_append packs the kept cubes of one vv_stream_cut round
// (vv_stream.hip) behind the cubes of the rounds before it in ONE large training store, so that a camera's frames become the store
// train.train_block trains from without the host asking after any frame.  It goes behind the round's cut on the same stream.
//
// One workgroup per slot b of the round.  The workgroup counts keep[0..b) itself (strided per-thread counts, LDS tree): that count is
// the slot's rank j among the kept slots, and its cube goes to store cube cursor_in[0] + j.  No workgroup waits for another and there
// are no atomics: every kept slot has a destination of its own.  Workgroup 0 alone also counts keep[0..n) and writes cursor_out[0] =
// cursor_in[0] + kept -- into ANOTHER cell than the one the other workgroups read, which is why the host alternates two cells.  The
// cursor is not clamped at the capacity (the host can say how many cubes the run would have needed); a cube whose destination lies at
// or past the capacity is not written anywhere.  A cube is copied with 16-byte loads and stores where source, destination and size
// allow (always for P = 32: 1024 * C * T bytes and 8192 * Tf bytes per cube, slots and stores 16-byte aligned), else byte by byte.
// Latency-bound: a round of 64 slots moves 3.6 MB at most.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vecvad_hip.h"
#include "vv_common.h"

namespace {

// bytes of one cube, by all 256 threads of the workgroup
__device__ __forceinline__ void copy_cube(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t bytes) {
  if ((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)bytes) & 15) == 0) {
    const uint4* s = (const uint4*)src;
    uint4* d = (uint4*)dst;
    for (int64_t i = threadIdx.x; i < bytes / 16; i += 256) d[i] = s[i];
  } else {
    for (int64_t i = threadIdx.x; i < bytes; i += 256) dst[i] = src[i];
  }
}

// keep[0..m) != 0, counted by the whole workgroup; every thread gets the count
__device__ __forceinline__ int count_kept(const uint8_t* __restrict__ keep, int m, int* part) {
  int c = 0;
  for (int i = threadIdx.x; i < m; i += 256) c += keep[i] != 0;
  part[threadIdx.x] = c;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  c = part[0];
  __syncthreads();                                       // part is used again
  return c;
}

__global__ void __launch_bounds__(256) stream_append_kernel(const uint8_t* __restrict__ raw_slots, const uint8_t* __restrict__ flow_slots,
                                                            const uint8_t* __restrict__ keep, const int32_t* __restrict__ n_ptr, int cap,
                                                            int64_t raw_bytes, int64_t flow_bytes, const uint8_t* __restrict__ masks,
                                                            int cells, const int32_t* __restrict__ boxes, int frame, int slot0,
                                                            const int32_t* __restrict__ cursor_in, int32_t* __restrict__ cursor_out,
                                                            int64_t capacity, uint8_t* __restrict__ raw_store,
                                                            uint8_t* __restrict__ flow_store, int32_t* __restrict__ meta,
                                                            int32_t* __restrict__ meta_boxes, uint8_t* __restrict__ meta_cells) {
  __shared__ int part[256];
  const int b = blockIdx.x;
  const int n = min(max(n_ptr[0], 0), cap);
  const int64_t cursor = cursor_in[0];
  if (b == 0) {                                          // the same for every thread of the workgroup, like every branch below
    const int kept = count_kept(keep, n, part);
    if (threadIdx.x == 0) cursor_out[0] = (int32_t)(cursor + kept);
  }
  if (b >= n || keep[b] == 0) return;
  const int64_t d = cursor + count_kept(keep, b, part);
  if (d < 0 || d >= capacity) return;                    // past the capacity (or a cursor nobody started at 0): not written anywhere
  copy_cube(raw_slots + (int64_t)b * raw_bytes, raw_store + d * raw_bytes, raw_bytes);
  copy_cube(flow_slots + (int64_t)b * flow_bytes, flow_store + d * flow_bytes, flow_bytes);
  for (int k = threadIdx.x; k < cells; k += 256) meta_cells[d * cells + k] = masks[(int64_t)k * cap + b];
  if (threadIdx.x == 0) {
    meta[2 * d] = frame;
    meta[2 * d + 1] = slot0 + b;
  }
  if (threadIdx.x < 4) meta_boxes[4 * d + threadIdx.x] = boxes ? boxes[4 * (int64_t)b + threadIdx.x] : 0;
}

}  // namespace

extern "C" int vv_stream_append(const uint8_t* raw_slots, const float* flow_slots, const uint8_t* keep, const int32_t* n, int32_t cap,
                                int64_t raw_cube_bytes, int64_t flow_cube_bytes, const uint8_t* masks, int32_t cells,
                                const int32_t* boxes, int32_t frame, int32_t slot0, const int32_t* cursor_in, int32_t* cursor_out,
                                int64_t capacity, uint8_t* raw_store, float* flow_store, int32_t* meta, int32_t* meta_boxes,
                                uint8_t* meta_cells, vv_stream stream) {
  if (cap < 1 || cells < 0 || capacity < 0 || raw_cube_bytes < 0 || flow_cube_bytes < 0) return VV_ERR_BAD_ARG;
  if (!n || !keep || !cursor_in || !cursor_out || cursor_in == cursor_out) return VV_ERR_BAD_ARG;
  if (!raw_slots || !flow_slots || !raw_store || !flow_store || !meta || !meta_boxes || !meta_cells) return VV_ERR_BAD_ARG;
  if (!masks && cells > 0) return VV_ERR_BAD_ARG;
  VV_LAUNCH(stream_append_kernel, dim3((unsigned)cap), dim3(256), 0, (hipStream_t)stream, raw_slots, (const uint8_t*)flow_slots, keep, n,
            cap, raw_cube_bytes, flow_cube_bytes, masks, cells, boxes, frame, slot0, cursor_in, cursor_out, capacity, raw_store,
            (uint8_t*)flow_store, meta, meta_boxes, meta_cells);
  VV_CHECK_LAUNCH();
  return VV_OK;
}
