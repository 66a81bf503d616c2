// mot_wave_sync.h — MOT_WAVE_SYNC alone, for mot_internal.h (every kernel file) and mot_wave.h (the primitives, mot_sort.h): no other dependency. Product code.
#ifndef MOT_WAVE_SYNC_H_
#define MOT_WAVE_SYNC_H_
// every lane of the wave has passed this point, and what it wrote to LDS before it is visible to the others (the emulator's lanes are fibers: a rendezvous)
#ifdef MOT_HIPEMU
#define MOT_WAVE_SYNC() ((void)__ballot(1))
#else
#define MOT_WAVE_SYNC()                                       \
  do {                                                        \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    \
    __builtin_amdgcn_wave_barrier();                          \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");    \
  } while (0)
#endif
#endif  // MOT_WAVE_SYNC_H_
