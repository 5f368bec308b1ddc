// Validation metrics of one batch in ONE launch: label-smoothed cross entropy, top-1 and top-k hits over the K selected
// classes of a (B, C) logit matrix, accumulated into five 64-bit words (the contract is in include/basd_hip.h).
//
// A streaming pass: B * K logits read from HBM once (the second pass over a row of at most a few KB is served by the
// caches), nothing written but the block's five atomic adds.  One wave per row, four rows per workgroup.  Pass 1: row
// maximum, rank of the target, NaN flag; pass 2: sum of exponentials and plain sum.  The loss is summed in fixed point
// (2^-32 units), so the state is the same bits whatever order the workgroups finish in: no hand-off between
// workgroups, nothing to wait for.
#include "basd_common.h"
#include "../../include/basd_hip.h"

namespace basd {

constexpr int kEvalRows = 4;             // waves (= rows) per workgroup
constexpr int kEvalBlock = kEvalRows * kWave;

typedef unsigned int v4u __attribute__((ext_vector_type(4)));

// element e of a 16-byte group: 4 fp32, or 8 bf16 (element 2w in the low half of word w)
template <typename T> struct EvalVec;
template <> struct EvalVec<float> {
    static constexpr int N = 4;
    static __device__ __forceinline__ float get(const v4u& r, int e) { return __uint_as_float(r[e]); }
};
template <> struct EvalVec<__hip_bfloat16> {
    static constexpr int N = 8;
    static __device__ __forceinline__ float get(const v4u& r, int e) {
        const unsigned w = r[e >> 1];
        return __uint_as_float((e & 1) ? (w & 0xffff0000u) : (w << 16));
    }
};

// f(j, z_j) for every selected class j of one row, the wave's lanes striding over them: 16-byte loads over the part of
// an aligned row that is taken in order, one element per lane and load otherwise (a class table, an odd row stride, the
// last K % N elements).  Returns false if the class table names a column outside [0, C): that column is not read.
template <typename T, typename F>
__device__ __forceinline__ bool eval_for_each(const T* __restrict__ x, const int* __restrict__ idx, int C, int K,
                                              int lane, bool vec, F&& f) {
    constexpr int N = EvalVec<T>::N;
    int done = 0;
    if (vec) {
        const int nv = K / N;
        for (int i = lane; i < nv; i += kWave) {
            const v4u r = ((const v4u*)x)[i];
#pragma unroll
            for (int e = 0; e < N; ++e) f(i * N + e, EvalVec<T>::get(r, e));
        }
        done = nv * N;
    }
    bool ok = true;
    for (int j = done + lane; j < K; j += kWave) {
        int c = j;
        if (idx) {
            c = idx[j];
            if ((unsigned)c >= (unsigned)C) { ok = false; continue; }
        }
        f(j, to_f32(x[c]));
    }
    return ok;
}

template <typename T>
__global__ void __launch_bounds__(kEvalBlock) eval_batch_kernel(const T* __restrict__ logits, long ld, int B, int C,
                                                                const int* __restrict__ class_index, int K,
                                                                const long* __restrict__ labels, float eps, int top_k,
                                                                long long* __restrict__ state) {
    __shared__ long long part[kEvalRows][5];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int b = blockIdx.x * kEvalRows + wid;
    long long fixed = 0;
    int rows = 0, hit1 = 0, hitk = 0, bad = 0;
    if (b < B) {                                             // wave-uniform
        const T* x = logits + (long)b * ld;
        const bool vec = class_index == nullptr && (((uintptr_t)x) & 15) == 0;
        const long y = labels[b];
        const bool y_ok = y >= 0 && y < K;
        bool ok = y_ok;
        float zy = 0.f;
        if (y_ok) {
            const int c = class_index ? class_index[y] : (int)y;
            if ((unsigned)c < (unsigned)C) zy = to_f32(x[c]);  // an index outside the row is reported by the pass below
        }
        const int yi = y_ok ? (int)y : 0;
        float m = -__builtin_inff();
        int ahead = 0;                                       // classes that rank before the target
        bool nan = false;
        ok &= eval_for_each(x, class_index, C, K, lane, vec, [&](int j, float z) {
            nan |= z != z;
            m = fmaxf(m, z);
            ahead += (z > zy || (z == zy && j < yi)) ? 1 : 0;
        });
        m = wave_max(m);
        ahead = wave_sum(ahead);
        ok &= __ballot(nan || !ok) == 0;
        float s = 0.f, sx = 0.f;
        eval_for_each(x, class_index, C, K, lane, vec, [&](int, float z) {
            const float v = z - m;
            s += expf(v);
            sx += v;
        });
        s = wave_sum(s);
        sx = wave_sum(sx);
        // -sum_j t'_j (v_j - lse), t' = (1 - eps) one-hot(y) + eps / K: the hard-label form of cross_entropy_kernel
        // (without smoothing the uniform part is left out, not multiplied by 0: a class masked with -inf costs nothing)
        float loss = logf(s) - (1.f - eps) * (zy - m);
        if (eps > 0.f) loss -= eps / (float)K * sx;
        ok &= fabsf(loss) < 16777216.f;                      // false for NaN and +-inf as well
        rows = 1;
        if (ok) {
            fixed = __double2ll_rn((double)loss * 4294967296.0);
            hit1 = ahead == 0;
            hitk = ahead < top_k;
        } else {
            bad = 1;
        }
    }
    if (lane == 0) {
        part[wid][0] = fixed;
        part[wid][1] = rows;
        part[wid][2] = hit1;
        part[wid][3] = hitk;
        part[wid][4] = bad;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < kEvalRows; ++w) v += part[w][threadIdx.x];
        if (v != 0) __hip_atomic_fetch_add(state + threadIdx.x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace basd

extern "C" {

int basd_eval_batch(const void* logits, int dtype, long ld, int B, int C, const int* class_index, int K,
                    const long* labels, float label_smoothing, int top_k, long long* state, hipStream_t stream) {
    BASD_CHECK_ARG(B >= 0 && C > 0 && K > 0 && top_k >= 1 && top_k <= K && state);
    BASD_CHECK_ARG(class_index != nullptr || K == C);
    BASD_CHECK_ARG(dtype == BASD_DTYPE_F32 || dtype == BASD_DTYPE_BF16);
    if (B == 0) return BASD_OK;
    BASD_CHECK_ARG(logits && labels && ld >= 0);
    const int grid = (B + basd::kEvalRows - 1) / basd::kEvalRows;
    if (dtype == BASD_DTYPE_F32) {
        // 16-byte loads need every row start on a 16-byte boundary: decided per row from its address, which covers ld
        basd::eval_batch_kernel<float><<<grid, basd::kEvalBlock, 0, stream>>>(
            (const float*)logits, ld, B, C, class_index, K, labels, label_smoothing, top_k, state);
    } else {
        basd::eval_batch_kernel<__hip_bfloat16><<<grid, basd::kEvalBlock, 0, stream>>>(
            (const __hip_bfloat16*)logits, ld, B, C, class_index, K, labels, label_smoothing, top_k, state);
    }
    BASD_RETURN_LAST();
}

}  // extern "C"
