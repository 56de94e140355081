// pcr_batch.h -- the entry points and the host launcher of every batched stage.
//
// A stage is one Op: its argument struct, its workgroup size and its device body,
//
//     struct OpScanCount : PcrOp<ScanArgs, BS> { __device__ static inline void run(const ScanArgs &a) { ... } };
//
// and PCR_BATCH_LAUNCH(ctx, OpScanCount, args, count, grid) runs `count` problems in one launch: blockIdx.y picks the problem, grid.y = count.
// Up to Op::kByValue problems (the scales of a multiscale registration, or one problem: a single call is a batch of one) carry their
// argument structs in the kernel arguments; larger batches (the clouds and scales of a GROUP of pairs) read them from the context's
// descriptor buffer (pcr_desc_upload: pinned staging -> device, one small asynchronous copy on the launch stream).
#pragma once
#include <cstring>
#include "pcr_internal.h"

#define PCR_MAX_BATCH 8            // problems whose argument structs travel in the kernel arguments
#define PCR_MAX_GROUP_BATCH 256    // problems of one launch in all
#define PCR_KERNARG_BYTES 4096     // what the kernel arguments of one launch may hold

template <class A, int N = PCR_MAX_BATCH> struct PcrBatch { A a[N]; };

// base of an Op.  kByValue: PCR_MAX_BATCH, or as many argument structs as the kernel arguments hold.  kWavesMin / kWavesMax: the
// amdgpu_waves_per_eu bounds of the entry points (0, 0: none); an Op that wants them declares its own.
template <class A, int THREADS> struct PcrOp {
    using Args = A;
    static constexpr int kThreads = THREADS;
    static constexpr int kByValue = sizeof(A) * PCR_MAX_BATCH <= PCR_KERNARG_BYTES ? PCR_MAX_BATCH : (int)(PCR_KERNARG_BYTES / sizeof(A));
    static constexpr int kWavesMin = 0, kWavesMax = 0;
};

// (the body is inlined by force: left to the inliner, whether it was inlined depended on the order in which the templates were
// instantiated, and a call out of line costs a stack frame and up to 100 VGPRs)
template <class Op> __global__ void __launch_bounds__(Op::kThreads) __attribute__((amdgpu_waves_per_eu(Op::kWavesMin, Op::kWavesMax)))
k_batch_value(PcrBatch<typename Op::Args, Op::kByValue> b) { [[clang::always_inline]] Op::run(b.a[blockIdx.y]); }
template <class Op> __global__ void __launch_bounds__(Op::kThreads) __attribute__((amdgpu_waves_per_eu(Op::kWavesMin, Op::kWavesMax)))
k_batch_pointer(const typename Op::Args *a) { [[clang::always_inline]] Op::run(a[blockIdx.y]); }

template <class Op>
static int pcr_batch_launch(pcr_context *ctx, const char *file, int line, const typename Op::Args *args, int count, dim3 grid) {
    using A = typename Op::Args;
    using B = PcrBatch<A, Op::kByValue>;
    static_assert(Op::kByValue >= 1 && sizeof(B) <= PCR_KERNARG_BYTES, "the by-value batch must fit the kernel arguments");
    if (count <= Op::kByValue) {
        B b; std::memset(&b, 0, sizeof b);
        for (int k = 0; k < count; k++) b.a[k] = args[k];
        pcr_launch(ctx, file, line, k_batch_value<Op>, grid, dim3(Op::kThreads), 0, ctx->stream, b);
    } else {
        const A *dev = pcr_desc_upload(ctx, args, count);
        if (!dev) return PCR_ENOMEM;
        pcr_launch(ctx, file, line, k_batch_pointer<Op>, grid, dim3(Op::kThreads), 0, ctx->stream, dev);
    }
    return PCR_OK;
}
#define PCR_BATCH_LAUNCH(ctx, Op, args, count, grid) pcr_batch_launch<Op>(ctx, __FILE__, __LINE__, args, count, grid)
