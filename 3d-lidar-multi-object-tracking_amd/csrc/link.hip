// link.hip — per-point track ids on gfx950. Product code (HIP, wave64).
//
// The last link of the chain the fused path already holds per slot: elevated point -> Cartesian cell (the 2 bytes the compaction kernel left beside the
// cloud) -> cluster label (the 16-bit label grid) -> box (box_cluster, written by the box stage's last kernel) -> owning track (the tracker's owner row,
// track.hip "box owners"). The reference has no such output: its tracker sees box centres only and throws matchingVec away (imm_ukf_jpda.cpp:806).
//
// A streaming kernel, grid (ceil(N_e / 2048), B), 256 threads, 8 points per thread as two quads: per quad one 8-byte load of four cells, four 2-byte gathers
// from the label grid (the label kernel's access pattern: a frame's occupied lines of the grid), four LDS reads, one 16-byte store of four ids. Every
// workgroup first builds the frame's cluster -> owner table in LDS (at most 4096 + 1 entries, 16 KB) from the slot's box_cluster and owner rows: two
// coalesced reads of at most 4 KB each, no atomics — a cluster has at most one box, so no two threads write the same entry. Nothing depends on the order
// in which workgroups or waves run. Algorithmic bytes per elevated point: 2 read, 4 written, plus the label gather.
#include "mot_internal.h"

#ifndef MOT_HIPEMU
#define MOT_LAUNCH_BOUNDS(n) __launch_bounds__(n)
#else
#define MOT_LAUNCH_BOUNDS(n)
#endif

constexpr int kLinkBlock = 256;
static_assert(kLinkChunk == kLinkBlock * 8, "two quads of points per thread");

__global__ void MOT_LAUNCH_BOUNDS(kLinkBlock)
point_tracks_kernel(MotDevParams p, ClusterBuffers c, const int* __restrict__ owner, int* __restrict__ ids, long id_stride, int* __restrict__ n_out) {
  __shared__ int s_own[kMaxClusters + 1];   // owner of the box of cluster (label) l, -1: no box or no owner; entry 0 = "no cluster"
  const int b = blockIdx.y, tid = threadIdx.x;
  const int* __restrict__ cnt = c.counts + (long)b * kCountsStride;
  const int n = cnt[kCntElev];
  if (blockIdx.x == 0 && tid == 0 && n_out) n_out[b] = n;
  const long lim = n < id_stride ? n : id_stride;   // points beyond the caller's stride are not written
  const long base = (long)blockIdx.x * kLinkChunk;
  if (base >= lim) return;   // (uniform over the workgroup)
  // a frame the box stage refused (capacity flags) has a cut or empty box list and, past the cluster limit, no label grid to speak of: every point reads -1
  const bool refused = cnt[kCntFlags] != 0;
  int nc = refused ? 0 : cnt[kCntClusters];
  nc = nc < 0 ? 0 : (nc > kMaxClusters ? kMaxClusters : nc);
  int M = refused ? 0 : cnt[kCntBoxes];
  M = M < 0 ? 0 : (M > kMaxBoxesPerFrame ? kMaxBoxesPerFrame : M);
  for (int l = tid; l <= nc; l += kLinkBlock) s_own[l] = -1;
  __syncthreads();
  for (int i = tid; i < M; i += kLinkBlock) {
    const int l = c.box_cluster[(long)b * kMaxBoxesPerFrame + i];
    if (l >= 1 && l <= nc) s_own[l] = owner[(long)b * kMaxBoxesPerFrame + i];
  }
  __syncthreads();
  const GridLabel* __restrict__ grid = c.grid + (long)b * (MOT_MAX_GRID * MOT_MAX_GRID);
  const unsigned short* __restrict__ ecell = c.ecell ? c.ecell + (long)b * c.cap : nullptr;
  int* __restrict__ out = ids + (long)b * id_stride;
  const bool vec_out = ((reinterpret_cast<uintptr_t>(out) & 15) == 0);   // the library's own buffer always; a caller's block when its slot starts on 16 bytes
#pragma unroll
  for (int r = 0; r < 2; r++) {
    const long i0 = base + ((long)r * kLinkBlock + tid) * 4;
    if (i0 >= lim) continue;
    const int valid = lim - i0 < 4 ? (int)(lim - i0) : 4;
    int id[4];
    if (ecell) {
      // four cells in one load (a slot's cells start on a multiple of 128 bytes, i0 is a multiple of 4; the slot holds cap >= i0 + 4 entries: cap is a multiple of 64)
      const uint2 q = *reinterpret_cast<const uint2*>(ecell + i0);
      const unsigned e[4] = {q.x & 0xffffu, q.x >> 16, q.y & 0xffffu, q.y >> 16};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        int lab = 0;
        if (j < valid && e[j] != 0xffffu) lab = (int)grid[(e[j] >> 8) * (unsigned)p.num_grid + (e[j] & 255u)];
        id[j] = (lab >= 1 && lab <= nc) ? s_own[lab] : -1;
      }
    } else {   // no cell codes (a 256-cell grid uses all 65536 of them): the cell from the point, as the label kernel does
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int lab = j < valid ? mot_point_label(p, c, b, i0 + j, nc) : 0;
        id[j] = lab >= 1 ? s_own[lab] : -1;
      }
    }
    if (valid == 4 && vec_out) *reinterpret_cast<int4*>(out + i0) = make_int4(id[0], id[1], id[2], id[3]);
    else {
#pragma unroll
      for (int j = 0; j < 4; j++) if (j < valid) out[i0 + j] = id[j];
    }
  }
}

void mot_launch_point_tracks(const MotDevParams& p, const ClusterBuffers& c, const int* owner, int batch, int max_n, int* ids, long id_stride, int* n_out, hipStream_t stream) {
  int chunks = (max_n + kLinkChunk - 1) / kLinkChunk;
  if (chunks < 1) chunks = 1;   // (workgroup 0 of a frame also reports its count)
  hipLaunchKernelGGL(point_tracks_kernel, dim3(chunks, batch), dim3(kLinkBlock), 0, stream, p, c, owner, ids, id_stride, n_out);
}
