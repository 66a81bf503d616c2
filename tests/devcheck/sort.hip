// sort.hip — the device-wide radix sort of csrc/mot_sort.h, driven directly. TEST INFRASTRUCTURE: a library of its own (tests/devcheck/libmot_sort.so for gfx950,
// libmot_sort_emu.so for the host; built by tests/devcheck/build_sort.py), like primitives.hip. It includes the product's header, so it runs the very kernels
// libmot_hip.so holds.
//   mot_sort_check   keys [n] and payloads [n] (host pointers) through mot_sort_launch over `key_bits` bits with buffers of `cap` elements; the count travels in
//                    device memory as the kernels read it. Synchronous on the null stream; returns 0, 1 (bad argument) or 3 (a HIP call failed).
// The cases and their reference (np.argsort(kind="stable")) are in tests/sort_cases.py.
#include <string.h>

#include "mot_sort.h"

#ifdef MOT_HIPEMU
__attribute__((used)) __shared__ int hipemu_lds_anchor;   // the emulator's launcher clears the "mot_lds" section: it has to exist in every library built against it
#endif

extern "C" __attribute__((visibility("default"))) int mot_sort_tile() { return kSortTile; }

extern "C" __attribute__((visibility("default"))) int mot_sort_check(const unsigned long long* keys, const unsigned* vals, int n, int cap, int key_bits,
                                                                       unsigned long long* keys_out, unsigned* vals_out) {
  if (!keys || !vals || !keys_out || !vals_out || n < 0 || cap < 1 || key_bits < 1 || key_bits > 64) return 1;
  const int live = n < cap ? n : cap;
  void* blocks[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const size_t bytes[7] = {8 * (size_t)cap, 8 * (size_t)cap, 4 * (size_t)cap, 4 * (size_t)cap, 4 * (size_t)kSortBins * mot_sort_tiles(cap), 4 * (size_t)kSortBins, 4};
  bool ok = true;
  for (int k = 0; k < 7 && ok; k++) ok = hipMalloc(&blocks[k], bytes[k]) == hipSuccess;
  if (ok) ok = hipMemcpy(blocks[0], keys, 8 * (size_t)live, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(blocks[2], vals, 4 * (size_t)live, hipMemcpyHostToDevice) == hipSuccess &&
               hipMemcpy(blocks[6], &n, 4, hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    SortBuffers b;
    b.key[0] = static_cast<unsigned long long*>(blocks[0]); b.key[1] = static_cast<unsigned long long*>(blocks[1]);
    b.val[0] = static_cast<unsigned*>(blocks[2]); b.val[1] = static_cast<unsigned*>(blocks[3]);
    b.table = static_cast<int*>(blocks[4]); b.totals = static_cast<int*>(blocks[5]); b.n = static_cast<const int*>(blocks[6]); b.cap = cap;
    const int at = mot_sort_launch(b, key_bits, 0);
    ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    if (ok && live) ok = hipMemcpy(keys_out, b.key[at], 8 * (size_t)live, hipMemcpyDeviceToHost) == hipSuccess &&
                         hipMemcpy(vals_out, b.val[at], 4 * (size_t)live, hipMemcpyDeviceToHost) == hipSuccess;
  }
  for (int k = 0; k < 7; k++) if (blocks[k]) (void)hipFree(blocks[k]);
  return ok ? 0 : 3;
}
