// Timing-only and A/B builds of the describe kernel (mkd_describe.hip), in one place.
//
// A PRODUCT build defines none of the macros below: every switch is then `false`, every hook a no-op that folds away, and
// the kernel source itself carries no preprocessor conditionals -- it reads as the product.  An instrument build
// (tools/ab_build.sh NAME "-DLF_ABLATE_MMA", tools/phase_timing.py, ...) flips one of them; such a build produces WRONG
// descriptors by design and exists only to be timed (NOTEBOOK.md sections 4, 9, 10 quote what they measured).
//
//   LF_ABLATE_BLOAD        no LUT fragment reads from LDS            LF_ABLATE_SPLIT     no f16 hi / lo split of the streams
//   LF_ABLATE_MMA          no matrix instructions (operands kept)    LF_ABLATE_FRONT     no blur, no gradient direction
//   LF_ABLATE_SYNC         no row barrier, no wait for the LDS-DMA   LF_ABLATE_EPILOGUE  no normalisation / whitening
//   LF_ABLATE_FORCE_W4     the 4-wave form at every request size
//   LF_ABLATE_ROW_DMA      patch mode: the row loop forms its LDS-DMA requests (raw rows, LUT rows) and issues none: every row
//                          computes on what the first requests of the launch left in LDS
//   LF_KP_ABLATE_PRODUCER  keypoint mode: the describe waves alone   LF_KP_ABLATE_TAPS   ... everything but a sample's loads
//   LF_KP_PRODUCER_PRIO=n / LF_KP_CONSUMER_PRIO=n                    wave priorities of the two kinds of wave
//   LF_ABLATE_ROWS=n       the row loop walks n of a patch's 32 rows (producers too): the bound of a row-split form.  Keypoint
//                          mode, and patch mode in F32 / F16_FP6; f16x3's patch mode walks row pairs and refuses to compile
//   LF_PHASE_TIMING        per-wave clocks of the phases of a patch row, left by workgroup 0 in out[wave * 128 + phase]
//   LF_WG_CLOCK            patch mode: entry and exit stamps, batch count and XCD of EVERY workgroup, left behind the descriptors
//                          (right descriptors: it times the product's walk over the batches, tools/wg_spread.py)
#pragma once
#include <hip/hip_runtime.h>

namespace lfmkd {
namespace ablate {

#ifdef LF_ABLATE_BLOAD
constexpr bool kNoFragmentReads = true;
#else
constexpr bool kNoFragmentReads = false;
#endif
#ifdef LF_ABLATE_SPLIT
constexpr bool kNoSplit = true;
#else
constexpr bool kNoSplit = false;
#endif
#ifdef LF_ABLATE_MMA
constexpr bool kNoMma = true;
#else
constexpr bool kNoMma = false;
#endif
#ifdef LF_ABLATE_FRONT
constexpr bool kNoFrontEnd = true;
#else
constexpr bool kNoFrontEnd = false;
#endif
#ifdef LF_ABLATE_MUL_FIRST_TAP   // the horizontal blur's first tap as a plain product (round 4's form: a blurred value can be -0.0)
constexpr bool kMulFirstTap = true;
#else
constexpr bool kMulFirstTap = false;
#endif
#ifdef LF_ABLATE_SYNC
constexpr bool kNoRowSync = true;
#else
constexpr bool kNoRowSync = false;
#endif
#ifdef LF_ABLATE_EPILOGUE
constexpr bool kNoEpilogue = true;
#else
constexpr bool kNoEpilogue = false;
#endif
#ifdef LF_ABLATE_FORCE_W4
constexpr bool kForceFourWaves = true;
#else
constexpr bool kForceFourWaves = false;
#endif
#ifdef LF_ABLATE_ROW_DMA   // the rows compute on what the first requests left in LDS: what the requests cost their issuer
constexpr bool kNoRowDma = true;
#else
constexpr bool kNoRowDma = false;
#endif
#ifdef LF_KP_ABLATE_PRODUCER
constexpr bool kNoProducer = true;
#else
constexpr bool kNoProducer = false;
#endif
#ifdef LF_KP_ABLATE_TAPS
constexpr bool kNoTaps = true;
#else
constexpr bool kNoTaps = false;
#endif
#ifdef LF_KP_PRODUCER_PRIO
constexpr int kProducerPrio = LF_KP_PRODUCER_PRIO;
#else
constexpr int kProducerPrio = 2;      // the product's setting (same-box A/B: +4 % over 0; NOTEBOOK.md 4f)
#endif
#ifdef LF_KP_CONSUMER_PRIO
constexpr int kConsumerPrio = LF_KP_CONSUMER_PRIO;
#else
constexpr int kConsumerPrio = -1;     // the describe waves keep the default priority
#endif

#ifdef LF_ABLATE_ROWS
constexpr int kRows = LF_ABLATE_ROWS;
#else
constexpr int kRows = 32;             // rows of a patch (lib.rs:15 PATCH_SIZE)
#endif

// ---- phase clocks ------------------------------------------------------------------------------------------------
#ifdef LF_PHASE_TIMING
constexpr bool kPhaseTiming = true;
#else
constexpr bool kPhaseTiming = false;
#endif
struct PhaseClock {
    unsigned long long clk[8] = {0, 0, 0, 0, 0, 0, 0, 0}, prev = 0;
    __device__ __forceinline__ void start() {
        if constexpr (kPhaseTiming) prev = __builtin_readcyclecounter();
    }
    // time since the previous mark goes to phase i
    __device__ __forceinline__ void mark(int i) {
        if constexpr (kPhaseTiming) {
            __builtin_amdgcn_sched_barrier(0);
            const unsigned long long t = __builtin_readcyclecounter();
            clk[i] += t - prev;
            prev = t;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // workgroup 0 leaves its waves' clocks where the descriptors would go (every wave of the workgroup calls)
    __device__ __forceinline__ void dump(float *out, int wave, int lane) const {
        if constexpr (kPhaseTiming) {
            __syncthreads();
            if (blockIdx.x == 0 && lane == 0)
                for (int i = 0; i < 8; ++i) out[wave * 128 + i] = (float)clk[i];
        }
    }
};

// ---- per-workgroup clock (patch mode) --------------------------------------------------------------------------------
// LF_WG_CLOCK: every workgroup stamps the constant 100 MHz clock on entry and after its last batch, counts its batches and
// reads its XCD; thread 0 leaves the record behind the descriptors, in out[n * 128 + 8 * workgroup ..] (eight 32-bit words:
// entry lo / hi, exit lo / hi, batches, XCD, 0, 0), so the caller's output holds 8 * grid floats more than n rows
// (tools/wg_spread.py).  The descriptors of such a build are the product's.
#ifdef LF_WG_CLOCK
constexpr bool kWgClock = true;
#else
constexpr bool kWgClock = false;
#endif
struct WgClock {
    unsigned batches = 0;
    __device__ __forceinline__ static unsigned *record(float *out, long n) {
        return reinterpret_cast<unsigned *>(out + n * 128) + 8 * (long)blockIdx.x;
    }
    __device__ __forceinline__ void enter(float *out, long n) const {
        if constexpr (kWgClock) {
            if (threadIdx.x == 0) {
                const unsigned long long t = __builtin_amdgcn_s_memrealtime();
                unsigned xcd;
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcd));
                unsigned *r = record(out, n);
                r[0] = (unsigned)t; r[1] = (unsigned)(t >> 32); r[5] = xcd; r[6] = 0u; r[7] = 0u;
            }
        }
    }
    __device__ __forceinline__ void batch_done() {
        if constexpr (kWgClock) ++batches;
    }
    // (every wave of the workgroup calls: the stamp is taken once all of them have left the last batch)
    __device__ __forceinline__ void leave(float *out, long n) const {
        if constexpr (kWgClock) {
            __syncthreads();
            if (threadIdx.x == 0) {
                const unsigned long long t = __builtin_amdgcn_s_memrealtime();
                unsigned *r = record(out, n);
                r[2] = (unsigned)t; r[3] = (unsigned)(t >> 32); r[4] = batches;
            }
        }
    }
};

}  // namespace ablate
}  // namespace lfmkd
