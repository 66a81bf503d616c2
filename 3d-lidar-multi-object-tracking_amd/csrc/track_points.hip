// track_points.hip — a frame's elevated points partitioned by owning track, on gfx950. Product code (HIP, wave64).
//
// mot_set_track_links left every elevated point with the id of the track that owns its cluster (link.hip). The kernels here turn "which track" into "that
// track's points": a STABLE sort of the frame's N_e points by a small key — the rank of the point's id among the distinct ids of the step's owner row, the
// points without owner (id -1) last — written as 16-byte records {x, y, z, index} into the caller's block, and the table of segments beside it. The reference
// has no such output (it never links a point to a track: link.hip's header).
//
//   P0  track_points_table_kernel    one workgroup per frame: the owner row (<= 1024 boxes, ids repeat when a track claimed several boxes) -> its distinct ids
//                                    >= 0 in ascending order and the boxes of each, by counting in LDS (rank of an id = distinct smaller ids)
//   P1  track_points_count_kernel    1024-point chunks: key of every point (binary search of its id in the frame's table, LDS) -> the chunk's points per key
//   P2  track_points_scan_kernel     one workgroup per frame: points per key over the chunks -> where each segment starts and where each chunk's points of each
//                                    key go; writes the segment table and the two true counts
//   P3  track_points_scatter_kernel  1024-point chunks: the key again, the point's rank among the chunk's points of its key, one 16-byte record per point
//
// One pass instead of regroup.hip's two digit passes: a key has at most 1025 values, so one LDS entry per key holds where the next point of the key goes and
// the place of a point is known after ONE look at the ids: (first record of its segment) + (points of its key in earlier chunks) + (... in earlier tiles of
// its chunk) + (lower lanes of its tile that hold the key). The last term comes from wave ballots on the key's bits, as in regroup.hip; the third from the
// four waves of a workgroup walking the chunk's 16 tiles four at a time, in order. No global atomics, nothing depends on the order in which workgroups or
// waves run, and the counts of the segment table are the very numbers the scatter places by. Only the first (distinct ids + 1) entries of a chunk's row are
// touched, in LDS and in memory.
// Bytes per elevated point: P1 4 read (id); P3 4 (id) + 12 (point) read, 16 written: 20 read + 16 written = 36, plus 3 x 4 (keys + 1) bytes per 1024-point
// chunk for the rows (about 0.5 bytes a point at 40 tracks, 12 at the limit of 1024). A plain copy of ids and points into such records moves 32.
#include "mot_track_place.h"   // the chunk geometry, the key of a point and P3's placement body (shared with track_accum.hip)

// ------------------------------------------------------------------------------------------ P0
__global__ void MOT_TP_BOUNDS(kTpBlock)
track_points_table_kernel(TrackPointBuffers t, int b0) {
  __shared__ int s_own[kMaxBoxesPerFrame];
  __shared__ int s_first[kMaxBoxesPerFrame];   // 1: the first box of the row that carries this id
  __shared__ int s_n;
  const int b = b0 + blockIdx.x, tid = threadIdx.x;
  const int M = mot_owner_boxes(t.counts, b);
  if (tid == 0) s_n = 0;
  for (int i = tid; i < M; i += kTpBlock) s_own[i] = t.owner[(long)b * kMaxBoxesPerFrame + i];
  __syncthreads();
  for (int i = tid; i < M; i += kTpBlock) {
    const int v = s_own[i];
    int first = v >= 0 ? 1 : 0;
    for (int j = 0; j < i && first; j++) first = s_own[j] != v;
    s_first[i] = first;
  }
  __syncthreads();
  int mine = 0;
  for (int i = tid; i < M; i += kTpBlock) {
    if (!s_first[i]) continue;
    const int v = s_own[i];
    int rank = 0, boxes = 0;
    for (int j = 0; j < M; j++) { const int w = s_own[j]; rank += (s_first[j] && w < v) ? 1 : 0; boxes += w == v ? 1 : 0; }
    t.seg_id[(long)b * kMaxBoxesPerFrame + rank] = v;      // (distinct ids: no two threads share a rank)
    t.seg_boxes[(long)b * kMaxBoxesPerFrame + rank] = boxes;
    mine++;
  }
  if (mine) atomicAdd(&s_n, mine);   // (LDS; an integer sum)
  __syncthreads();
  if (tid == 0) t.seg_n[b] = s_n;
}

// ------------------------------------------------------------------------------------------ P1
__global__ void MOT_TP_BOUNDS(kTpBlock)
track_points_count_kernel(TrackPointBuffers t, int b0) {
  __shared__ int s_ids[kMaxBoxesPerFrame];
  __shared__ int s_hist[kTrackPointKeys];
  const int b = b0 + blockIdx.y, tid = threadIdx.x;
  const int n = tp_count(t, b);
  const long base = (long)blockIdx.x * kTrackPointChunk;
  if (base >= n || (int)blockIdx.x >= t.max_chunks) return;
  const int R = tp_segments(t, b);
  for (int j = tid; j <= R; j += kTpBlock) { s_hist[j] = 0; if (j < R) s_ids[j] = t.seg_id[(long)b * kMaxBoxesPerFrame + j]; }
  __syncthreads();
  const int* __restrict__ ids = t.ids + (long)b * t.cap;
  int bits = 0;
  while ((R >> bits) != 0) bits++;   // keys 0 .. R
  const unsigned long long below = (1ull << (tid & 63)) - 1ull;
#pragma unroll
  for (int k = 0; k < kTpItems; k++) {
    const long i = base + k * kTpBlock + tid;
    const int key = i < n ? tp_key(ids[i], s_ids, R) : 0;
    // one LDS add per (tile, key) instead of one per point: the points of a frame share a handful of keys, and adds to one address take turns
    unsigned long long same = __ballot(i < n);
    for (int bit = 0; bit < bits; bit++) {
      const unsigned long long set = __ballot((key >> bit) & 1);
      same &= ((key >> bit) & 1) ? set : ~set;
    }
    if (i < n && (same & below) == 0) atomicAdd(&s_hist[key], __popcll(same));
  }
  __syncthreads();
  int* __restrict__ row = t.rows + ((long)b * t.max_chunks + blockIdx.x) * kTrackPointKeys;
  for (int j = tid; j <= R; j += kTpBlock) row[j] = s_hist[j];
}

// ------------------------------------------------------------------------------------------ P2
// rows[chunk][key] (counts) -> the place of the chunk's first point of that key: the records of all smaller keys, then the key's points of earlier chunks.
// Keys tid, tid + 256, ... per thread (consecutive threads read consecutive words of a row). The segment table and the counts of slot k of the caller's block.
__global__ void MOT_TP_BOUNDS(kTpBlock)
track_points_scan_kernel(TrackPointBuffers t, int b0, int rest, mot_track_segment* __restrict__ segs, int max_segments, int* __restrict__ counts_out) {
  constexpr int kPer = (kTrackPointKeys + kTpBlock - 1) / kTpBlock;   // 5
  __shared__ int s_part[kTpBlock / 64];
  const int k = blockIdx.x, b = b0 + k, tid = threadIdx.x;
  const int chunks = tp_chunks(t, b);
  const int R = tp_segments(t, b);
  int* __restrict__ rows = t.rows + (long)b * t.max_chunks * kTrackPointKeys;
  mot_track_segment* __restrict__ out = segs + (long)k * max_segments;
  const bool vec_out = ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  int carry = 0;   // records of the keys of earlier rounds
  for (int q = 0; q < kPer && q * kTpBlock <= R; q++) {   // (uniform)
    const int key = q * kTpBlock + tid;
    int sum = 0;
    if (key <= R) for (int ch = 0; ch < chunks; ch++) sum += rows[(long)ch * kTrackPointKeys + key];
    // exclusive prefix over the round's 256 keys (block_scan_excl_i32, mot_wave.h)
    int total;
    const int first = carry + block_scan_excl_i32<kTpBlock / 64>(sum, s_part, total);
    carry += total;
    __syncthreads();   // (s_part is written again in the next round)
    if (key > R) continue;
    int run = first;
    for (int ch = 0; ch < chunks; ch++) {
      const int v = rows[(long)ch * kTrackPointKeys + key];
      rows[(long)ch * kTrackPointKeys + key] = run;
      run += v;
    }
    const bool is_rest = key == R;
    if (is_rest && counts_out) { counts_out[2 * k] = R + (rest ? 1 : 0); counts_out[2 * k + 1] = rest ? first + sum : first; }
    if ((is_rest && !rest) || key >= max_segments) continue;
    const int id = is_rest ? -1 : t.seg_id[(long)b * kMaxBoxesPerFrame + key];
    const int boxes = is_rest ? 0 : t.seg_boxes[(long)b * kMaxBoxesPerFrame + key];
    if (vec_out) *reinterpret_cast<int4*>(out + key) = make_int4(id, first, sum, boxes);
    else { int* o = reinterpret_cast<int*>(out + key); o[0] = id; o[1] = first; o[2] = sum; o[3] = boxes; }
  }
}

// ------------------------------------------------------------------------------------------ P3
// The placement is tp_place_chunk (mot_track_place.h); the sink here is the caller's block: place = the record's index in the slot's block.
struct TpExportSink {
  mot_track_point* __restrict__ out;
  long lim;       // records beyond the caller's stride are not written
  bool vec_out;
  __device__ __forceinline__ bool takes(int, long dst) const { return dst < lim; }   // (dst < n while the rows are this frame's; never a store outside the slot's records)
  __device__ __forceinline__ void put(int, long dst, float4 o, long i) const {
    o.w = __int_as_float((int)i);
    if (vec_out) *reinterpret_cast<float4*>(out + dst) = o;
    else { float* p = reinterpret_cast<float*>(out + dst); p[0] = o.x; p[1] = o.y; p[2] = o.z; p[3] = o.w; }
  }
};
__global__ void MOT_TP_BOUNDS(kTpBlock)
track_points_scatter_kernel(TrackPointBuffers t, int b0, int rest, const EgoTf* __restrict__ tf, mot_track_point* __restrict__ points, long point_stride) {
  MOT_TP_PLACE_LDS(s);
  const int kb = blockIdx.y, b = b0 + kb;
  const int n = tp_count(t, b);
  mot_track_point* out = points + (long)kb * point_stride;
  const TpExportSink sink = {out, n < point_stride ? n : point_stride, (reinterpret_cast<uintptr_t>(out) & 15) == 0};
  tp_place_chunk(t, b, kb, rest, tf, s, sink);
}

// ------------------------------------------------------------------------------------------ host
void mot_launch_track_point_counts(const TrackPointBuffers& t, int first, int batch, int max_n, hipStream_t stream) {
  const int chunks = mot_launch_chunks(max_n, kTrackPointChunk, t.max_chunks);
  hipLaunchKernelGGL(track_points_table_kernel, dim3(batch), dim3(kTpBlock), 0, stream, t, first);
  hipLaunchKernelGGL(track_points_count_kernel, dim3(chunks, batch), dim3(kTpBlock), 0, stream, t, first);
}
void mot_launch_track_points(const TrackPointBuffers& t, int first, int batch, int max_n, int rest, const EgoTf* tf, mot_track_point* points, long point_stride,
                             mot_track_segment* segs, int max_segments, int* counts_out, hipStream_t stream) {
  const int chunks = mot_launch_chunks(max_n, kTrackPointChunk, t.max_chunks);
  const dim3 grid(chunks, batch);
  mot_launch_track_point_counts(t, first, batch, max_n, stream);
  hipLaunchKernelGGL(track_points_scan_kernel, dim3(batch), dim3(kTpBlock), 0, stream, t, first, rest, segs, max_segments, counts_out);
  hipLaunchKernelGGL(track_points_scatter_kernel, grid, dim3(kTpBlock), 0, stream, t, first, rest, tf, points, point_stride);
}
