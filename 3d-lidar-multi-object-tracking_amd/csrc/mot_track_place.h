// mot_track_place.h — what the kernels that walk a frame's elevated points by owning track share: track_points.hip (the partition into the caller's block) and
// track_accum.hip (the append to the per-track rings). The geometry of a chunk, the key of a point, and the IN-ORDER PLACEMENT of a chunk's points: the body of
// track_points.hip's P3, with the place a point's record goes to left to a sink. One body, two sinks — the export stays byte for byte what it was, and the rings
// get the same input-order guarantee from the same code.
#ifndef MOT_TRACK_PLACE_H_
#define MOT_TRACK_PLACE_H_
#include "mot_internal.h"
#include "mot_wave.h"

#ifndef MOT_HIPEMU
#define MOT_TP_BOUNDS(n) __launch_bounds__(n)
#else
#define MOT_TP_BOUNDS(n)
#endif

constexpr int kTpBlock = 256, kTpItems = kTrackPointChunk / kTpBlock;
constexpr int kTpTiles = kTrackPointChunk / 64;
constexpr int kTpWaves = kTpBlock / 64;
static_assert(kTrackPointChunk % kTpBlock == 0 && kTpItems * (kTpBlock / 64) == kTpTiles, "a wave takes one 64-point tile per item");
static_assert(sizeof(mot_track_point) == 16 && sizeof(mot_track_segment) == 16, "one 16-byte store per record");

// the frame's elevated points and boxes as every kernel here sees them (never beyond the slot: the counts are the device's)
__device__ __forceinline__ int tp_count(const TrackPointBuffers& t, int b) {
  const int n = t.counts[b * kCountsStride + kCntElev];
  return n < 0 ? 0 : (n < (int)t.cap ? n : (int)t.cap);
}
// ... and the chunks of them that t.rows has a row for
__device__ __forceinline__ int tp_chunks(const TrackPointBuffers& t, int b) {
  const int chunks = (tp_count(t, b) + kTrackPointChunk - 1) / kTrackPointChunk;
  return chunks > t.max_chunks ? t.max_chunks : chunks;
}
__device__ __forceinline__ int tp_segments(const TrackPointBuffers& t, int b) {
  const int r = t.seg_n[b];
  return r < 0 ? 0 : (r < kMaxBoxesPerFrame ? r : kMaxBoxesPerFrame);
}
// rank of `id` among the frame's R distinct owners (ascending in s_ids); R for a point without owner
__device__ __forceinline__ int tp_key(int id, const int* s_ids, int R) {
  if (id < 0) return R;
  int lo = 0, hi = R;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_ids[mid] < id) lo = mid + 1; else hi = mid; }
  return (lo < R && s_ids[lo] == id) ? lo : R;   // (every id >= 0 the link kernel wrote is in the row it read)
}

// the LDS of a placement workgroup, declared by the kernel that calls tp_place_chunk (16 464 bytes with their padding)
struct TpPlaceLds {
  unsigned short (*cnt)[kTrackPointKeys];   // [kTpWaves] points of (tile of this step, key); zero between steps
  int* base;                                // [kTrackPointKeys]
  int* ids;                                 // [kMaxBoxesPerFrame]
  float* m;                                 // [12]
};
#define MOT_TP_PLACE_LDS(name)                                        \
  __shared__ unsigned short name##_cnt[kTpWaves][kTrackPointKeys];    \
  __shared__ int name##_base[kTrackPointKeys];                        \
  __shared__ int name##_ids[kMaxBoxesPerFrame];                       \
  __shared__ float name##_m[12];                                      \
  const TpPlaceLds name = {name##_cnt, name##_base, name##_ids, name##_m}

// A chunk is 16 tiles of 64 consecutive points; the workgroup's four waves take four consecutive tiles per step, in index order. s.base[key] is where the next
// point of a key goes — the chunk's entry of t.rows to begin with, whatever the kernel before left there: a record index of the caller's block (export), a rank
// within the key's segment (rings); within a step a point's place is s.base[key] + (points of the key in the step's lower tiles, s.cnt) + (lower lanes of its own
// tile that hold the key). After every step the lowest lane of each (tile, key) moves s.base on by its tile's count — LDS integer adds of one step, complete before
// the next step reads — and clears its entry. Ids and points of all four steps are loaded up front.
// Sink: takes(key, place) — is the record wanted there (uniform work is not required) — and put(key, place, {x, y, z, -}, i) stores point i's record. Keys < R, and
// key R (the points without owner) when rest != 0, reach the sink.
template <class Sink>
__device__ __forceinline__ void tp_place_chunk(const TrackPointBuffers& t, int b, int kb, int rest, const EgoTf* __restrict__ tf, const TpPlaceLds& s, const Sink& sink) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = tp_count(t, b);
  const long base = (long)blockIdx.x * kTrackPointChunk;
  if (base >= n || (int)blockIdx.x >= t.max_chunks) return;
  const int R = tp_segments(t, b);
  const int* __restrict__ row = t.rows + ((long)b * t.max_chunks + blockIdx.x) * kTrackPointKeys;
  for (int j = tid; j <= R; j += kTpBlock) {
    s.base[j] = row[j];
    if (j < R) s.ids[j] = t.seg_id[(long)b * kMaxBoxesPerFrame + j];
#pragma unroll
    for (int w = 0; w < kTpWaves; w++) s.cnt[w][j] = 0;
  }
  if (tf && tid < 12) s.m[tid] = tf[kb].m[tid];
  const int* __restrict__ ids = t.ids + (long)b * t.cap;
  int id[kTpItems];
  float4 q[kTpItems];
#pragma unroll
  for (int k = 0; k < kTpItems; k++) {
    const long i = base + k * kTpBlock + tid;
    id[k] = i < n ? ids[i] : -1;
    q[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n && (rest || id[k] >= 0)) q[k] = mot_load_xyz(t.elevated + (long)b * t.cap, i, t.elevated_packed);
  }
  __syncthreads();
  int bits = 0;
  while ((R >> bits) != 0) bits++;   // keys 0 .. R
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int k = 0; k < kTpItems; k++) {
    const long i = base + k * kTpBlock + tid;   // tile k * 4 + wave of the chunk: points 64 * tile .. 64 * tile + 63
    const bool valid = i < n;
    const int key = valid ? tp_key(id[k], s.ids, R) : 0;
    unsigned long long same = __ballot(valid);   // the lanes of this tile that hold my key
    for (int bit = 0; bit < bits; bit++) {
      const unsigned long long set = __ballot((key >> bit) & 1);
      same &= ((key >> bit) & 1) ? set : ~set;
    }
    const int rank = __popcll(same & below), mine = __popcll(same);
    const bool leader = valid && rank == 0;   // the lowest lane of each key present in the tile
    if (leader) s.cnt[wave][key] = (unsigned short)mine;
    __syncthreads();
    const bool wanted = valid && (key < R || rest);
    long dst = 0;
    if (wanted) {
      dst = s.base[key] + rank;
      for (int w = 0; w < wave; w++) dst += s.cnt[w][key];
    }
    __syncthreads();
    if (leader) { atomicAdd(&s.base[key], mine); s.cnt[wave][key] = 0; }
    if (!wanted || !sink.takes(key, dst)) continue;
    float4 o;
    if (tf) {   // fp32, left to right; the build has -ffp-contract=off (mot_track_prep.h's sensor -> global step, track.hip's way back)
      o.x = s.m[0] * q[k].x + s.m[1] * q[k].y + s.m[2] * q[k].z + s.m[3];
      o.y = s.m[4] * q[k].x + s.m[5] * q[k].y + s.m[6] * q[k].z + s.m[7];
      o.z = s.m[8] * q[k].x + s.m[9] * q[k].y + s.m[10] * q[k].z + s.m[11];
    } else { o.x = q[k].x; o.y = q[k].y; o.z = q[k].z; }
    o.w = 0.f;
    sink.put(key, dst, o, i);
  }
}

// P0 and P1 of track_points.hip over slots first .. first + batch - 1: the distinct owners of every frame and each chunk's points per key (t.seg_*, t.rows)
void mot_launch_track_point_counts(const TrackPointBuffers& t, int first, int batch, int max_n, hipStream_t stream);
#endif  // MOT_TRACK_PLACE_H_
