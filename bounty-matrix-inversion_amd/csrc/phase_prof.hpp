// Per-phase cycle counters of the blind-rotation kernels, in -DBMI_PHASE_PROF builds only (make -C csrc prof; tools/phase_prof*.py).
// Without the macro everything here expands to nothing: the product build contains none of it.
//
// A profiled translation unit declares its own array (device variables are per translation unit) and exports it under the name
// its tool calls:   PH_ARRAY(g_phase_x) in its unnamed namespace,   PH_EXPORT(bmi_debug_phase_prof_x, g_phase_x) at file scope.
// A profiled kernel:  PH_DECL() before its step loop,  PH_MARK(k) (k < 8) after each phase: the cycles since the last mark are
// added to counter k;  PH_STORE(g_phase_x, wave, lane) after the loop: lane 0 of every wavefront of workgroup 0 writes its
// eight counters to [wave][8].
#pragma once

#ifdef BMI_PHASE_PROF
#define PH_ARRAY(arr) __device__ unsigned long long arr[128];
#define PH_EXPORT(name, arr)                                                                                \
    extern "C" int name(unsigned long long *out128) {                                                       \
        return (int)hipMemcpyFromSymbol(out128, HIP_SYMBOL(arr), sizeof(unsigned long long) * 128);         \
    }
#define PH_DECL() unsigned long long ph_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tl_ = clock64()
#define PH_MARK(k)                               \
    do {                                         \
        const unsigned long long t_ = clock64(); \
        ph_[k] += t_ - tl_;                      \
        tl_ = t_;                                \
    } while (0)
#define PH_STORE(arr, wave, lane)                                             \
    do {                                                                      \
        if (blockIdx.x == 0 && (lane) == 0)                                   \
            for (int k_ = 0; k_ < 8; k_++) arr[(wave) * 8 + k_] = ph_[k_];    \
    } while (0)
#else
#define PH_ARRAY(arr)
#define PH_EXPORT(name, arr)
#define PH_DECL()
#define PH_MARK(k)
#define PH_STORE(arr, wave, lane)
#endif
