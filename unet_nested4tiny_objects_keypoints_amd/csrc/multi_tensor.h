// The multi-tensor launch: one kernel launch over many tensors of unrelated sizes.  The fused optimizer step, gradient
// clipping (optim.hip) and weight averaging (average.hip) all rest on it; the host side that builds and caches the
// table is multi_tensor.py.  THIS comment is the one description of the design; everything else points here.
//
// Table      one device buffer [segments | chunk -> segment map | arrival counter], filled in a page-locked host buffer
//            that lives as long as the table and uploaded asynchronously (unetpp_optim_upload).
//              segments   n_seg structs of the caller's type (unetpp_optim_segment, unetpp_avg_segment).  This header
//                         reads three fields: numel, chunk_begin and vec.  Tensors without elements have no segment.
//              map        int32 [n_chunks] at byte n_seg * sizeof(segment): the segment of every chunk.  Segment s owns
//                         the chunks [chunk_begin, chunk_begin + ceil(numel / 4096)), in segment order.
//              counter    8 bytes, zero, after the map (int32 used): only tables of capturable launches have one.
// Grid       persistent: min(n_chunks, 8 x CUs) workgroups of 256 threads; workgroup b takes chunks b, b + grid, ...
// Chunk walk chunk c of a segment covers its elements [begin, end) = [(c - chunk_begin) * 4096, min(.. + 4096, numel)).
//            vec (every stream of the segment 16-byte aligned): thread t takes the float4 at begin + (k * 256 + t) * 4,
//            k = 0..3, while it lies below vend = begin + ((end - begin) & ~3); the < 4 elements from vend, which only
//            a segment's last chunk has, go one per thread.  !vec: one element per thread from begin, stride 256.
//            Every element is visited exactly once and depends on no other, so the path does not change the bits.
// Arrival    capturable launches advance a device-side count AFTER every workgroup has read it: each workgroup adds 1
//            to the counter when it is done, the one that sees grid - 1 is the last, does the update and stores 0 for
//            the next launch.  Integer arrivals only: nothing floating-point depends on the order.
//
// No floating-point arithmetic here: optim.hip and average.hip switch implicit contraction off at file scope, and the
// arithmetic (the callables handed to walk_chunk) stays lexically inside those files, after their pragma.
#pragma once

#include "common.h"

namespace unetpp {

constexpr int kMtThreads = 256;
constexpr int kMtVecPerThread = 4;                                       // float4 per thread and stream
constexpr int64_t kMtChunk = int64_t(kMtThreads) * kMtVecPerThread * 4;   // 4096 elements

struct ChunkSpan {
  int64_t begin, end;   // elements of the segment
};

__device__ __forceinline__ ChunkSpan chunk_span(int64_t numel, int64_t chunk_begin, int64_t c) {
  const int64_t begin = (c - chunk_begin) * kMtChunk;
  return {begin, begin + kMtChunk < numel ? begin + kMtChunk : numel};
}

// where thread tid's k-th float4 of a chunk starts, in elements from the chunk's begin
__host__ __device__ constexpr int64_t vec_slot_offset(int k, unsigned tid) {
  return (int64_t(k) * kMtThreads + tid) * 4;
}

// f4(i): the aligned float4 at element i;  f1(i): the one element i
template <class F4, class F1>
__device__ __forceinline__ void walk_chunk(const ChunkSpan sp, bool vec, F4&& f4, F1&& f1) {
  int64_t tail = sp.begin;   // where the scalar loop starts
  if (vec) {
    const int64_t vend = sp.begin + ((sp.end - sp.begin) & ~int64_t(3));
#pragma unroll
    for (int k = 0; k < kMtVecPerThread; ++k) {
      const int64_t i = sp.begin + vec_slot_offset(k, threadIdx.x);
      if (i >= vend) break;
      f4(i);
    }
    tail = vend;   // < 4 elements: the segment's tail
  }
  for (int64_t i = tail + threadIdx.x; i < sp.end; i += kMtThreads) f1(i);
}

// true in every thread of the last workgroup of the grid to get here, once all the others have (see Arrival above);
// that workgroup stores 0 to *done when it has done its work
__device__ __forceinline__ bool last_workgroup(int32_t* done) {
  __shared__ int last;
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    last = atomicAdd(done, 1) == static_cast<int>(gridDim.x) - 1;
  }
  __syncthreads();
  return last;
}

inline unsigned persistent_grid(int64_t n_chunks) {
  const int cus = device_cu_count();
  const int64_t cap = int64_t(cus > 0 ? cus : 256) * 8;
  return static_cast<unsigned>(n_chunks < cap ? n_chunks : cap);
}

inline bool table_args_ok(const void* segments, int32_t n_segments, const int32_t* chunk_segment, int64_t n_chunks) {
  return segments != nullptr && n_segments > 0 && chunk_segment != nullptr && n_chunks > 0;
}

}  // namespace unetpp
