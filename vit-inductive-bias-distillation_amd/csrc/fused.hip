// One library call = one stage of the loss step.  The per-kernel entry points stay (tests and the general paths use
// them); these functions queue the same launches in the same order from C, because a dozen separate FFI calls from
// Python cost several times the launches themselves and that host time sits in front of the kernels of the caller's
// stream (round-1 timeline: the first Procrustes kernel started 1.05 ms into a 3.5 ms step).
#include "basd_common.h"
#include "procrustes_plan.h"

namespace basd {

// combined.py:76-85 on the device: per-layer means of loss_b (E, B), their mean, the UW-SO weights of (ce, geo) from the
// DETACHED values, the total.  One workgroup; means accumulated in fp64 in a fixed order.
__global__ void __launch_bounds__(256) uwso_combine_kernel(const float* __restrict__ ce, const float* __restrict__ loss_b,
                                                           int E, int B, float* __restrict__ out) {
    constexpr int CH = 32;                  // layers per pass: one barrier per pass, not two per layer
    __shared__ double red[CH][4];
    const int tid = threadIdx.x;
    double geo_sum = 0.;                    // thread 0 only
    for (int e0 = 0; e0 < E; e0 += CH) {
        const int ne = E - e0 < CH ? E - e0 : CH;
        for (int e = 0; e < ne; ++e) {
            double acc = 0.;
            for (int b = tid; b < B; b += 256) acc += (double)loss_b[(long)(e0 + e) * B + b];
            for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m, 64);
            if ((tid & 63) == 0) red[e][tid >> 6] = acc;
        }
        __syncthreads();
        if (tid == 0)
            for (int e = 0; e < ne; ++e) {
                const float layer = (float)(((red[e][0] + red[e][1]) + (red[e][2] + red[e][3])) / (double)B);
                out[4 + E + e0 + e] = layer;
                geo_sum += (double)layer;
            }
        __syncthreads();
    }
    if (tid == 0) {
        const float c = ce[0], geo = (float)(geo_sum / (double)E);
        const float eps = 1.1920929e-7f;                       // torch.finfo(float32).eps
        const float i0 = 1.f / fmaxf(c, eps), i1 = 1.f / fmaxf(geo, eps);
        const float w0 = i0 / (i0 + i1), w1 = i1 / (i0 + i1);
        out[0] = w0;
        out[1] = w1;
        out[2] = w0 * c + w1 * geo;
        out[3] = geo;
        for (int e = 0; e < E; ++e) out[4 + e] = w1 / (float)E;
    }
}

__global__ void __launch_bounds__(256) scale_unless_one_kernel(float* __restrict__ x, long count4, long count,
                                                               const float* __restrict__ num,
                                                               const float* __restrict__ den) {
    // grid-stride over a few workgroups per CU: when nothing is to be scaled (the common case) a handful of
    // workgroups read the factor once and leave, instead of one workgroup per 1024 elements
    const float f = den ? num[0] / den[0] : num[0];
    if (f == 1.f) return;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count4; i += (long)gridDim.x * 256) {
        float4 v = ((float4*)x)[i];
        v.x *= f; v.y *= f; v.z *= f; v.w *= f;
        ((float4*)x)[i] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(count - 4 * count4)) x[4 * count4 + threadIdx.x] *= f;
}

}  // namespace basd

extern "C" {

int basd_scale_unless_one(float* x, long count, const float* num, const float* den, hipStream_t stream) {
    BASD_CHECK_ARG(x && num && count > 0 && ((uintptr_t)x & 15) == 0);
    const long count4 = count / 4;
    const long groups = (count4 + 255) / 256 + (count4 == 0);
    basd::scale_unless_one_kernel<<<(unsigned)(groups < 1024 ? groups : 1024), 256, 0, stream>>>(x, count4, count, num, den);
    BASD_RETURN_LAST();
}

// Test hook: 0 keeps the stacked cores [M; L_b] (riding rows) for every shape, 2 drops the batch threshold.
static int g_transposed_cores = 1;
int basd_procrustes_tuning(int transposed_cores) {
    if (transposed_cores >= 0) g_transposed_cores = transposed_cores > 2 ? 2 : transposed_cores;
    return BASD_OK;
}
// Test / measurement hook: 0 keeps basd_procrustes_finalize + basd_kprime_from_transposed behind the transposed route's
// Jacobi, 1 (default) takes basd_procrustes_finish_transposed where it applies.  Returns the previous setting.
static int g_finish_fused = 1;
int basd_procrustes_finish_tuning(int fused) {
    const int prev = g_finish_fused;
    if (fused >= 0) g_finish_fused = fused ? 1 : 0;
    return prev;
}

// What basd_procrustes_forward_fused would launch for these arguments under the current hooks (host only, no HIP call;
// pointers are only tested for presence and alignment): the fields of basd::plan::ProcrustesPlan in order.
static int plan_query(const BasdProcrustesArgs* a, long* out20, bool teacher_given) {
    using namespace basd::plan;
    BASD_CHECK_ARG(out20);
    ProcrustesPlan p;
    BASD_TRY(procrustes_plan(a, g_transposed_cores, g_finish_fused, &p, teacher_given));
    const long out[kPlanFields] = {p.center, p.project, p.slab_width, p.slabs, p.gram_split, p.chol, p.cores,
                                   p.svd, p.finish, p.rebuild_usigma, p.grad, p.usigma_in, p.tr_part_floats,
                                   p.w_borrow_floats, p.lds_center, p.lds_project, p.lds_gram, p.lds_chol,
                                   p.lds_finish, p.lds_grad};
    for (int i = 0; i < kPlanFields; ++i) out20[i] = out[i];
    return p.status();
}
int basd_procrustes_plan_query(const BasdProcrustesArgs* a, long* out20) { return plan_query(a, out20, false); }
// The same for basd_procrustes_forward_cached: field 0 is 5 ("given"), fields 4, 13 and 14 are 0.
int basd_procrustes_plan_query_cached(const BasdProcrustesArgs* a, long* out20) { return plan_query(a, out20, true); }
// The same for basd_procrustes_teacher_side: fields 0, 4, 13, 14 and 16 as in basd_procrustes_plan_query, the rest 0.
int basd_procrustes_plan_query_teacher_side(const BasdProcrustesArgs* a, long* out20) {
    using namespace basd::plan;
    BASD_CHECK_ARG(out20);
    ProcrustesPlan p;
    BASD_TRY(teacher_side_plan(a, &p));
    for (int i = 0; i < kPlanFields; ++i) out20[i] = 0;
    out20[0] = p.center, out20[4] = p.gram_split, out20[13] = p.w_borrow_floats, out20[14] = p.lds_center;
    out20[16] = p.lds_gram;
    return p.teacher_status();
}

// The teacher half of the call, one statement of it for basd_procrustes_forward_fused and
// basd_procrustes_teacher_side, in the two pieces the uncached call queues around its student projection.
// Token weights + mixed, centred teacher, once per group (G = 1: shared by all layers), by the centring route of the plan.
static int teacher_weights_and_centring(const BasdProcrustesArgs* a, const basd::plan::ProcrustesPlan& p, hipStream_t st) {
    using namespace basd::plan;
    const int L = (int)a->L, G = (int)a->G, B = (int)a->B, n_s = (int)a->n_s, d_t = (int)a->d_t, n = (int)a->n;
    const int td = (int)a->t_dtype;
    for (int g = 0; g < G; ++g) {
        BASD_TRY(basd_token_weights(a->attn_ptrs, (int)a->a_dtype, a->mix + (long)g * L, L, a->a_sb, a->a_sh, a->a_sq,
                                    a->a_sk, B, (int)a->H, (int)a->A, (int)a->has_cls, (int)a->n_a, n, n_s, a->atap0,
                                    a->atap1, a->alam, a->tap0, a->tap1, a->lam, a->omega + (long)g * B * n_s,
                                    a->omega_t + (long)g * B * n, a->raw ? a->raw + (long)g * B * a->n_a : nullptr, st));
    }
    switch (p.center) {
        case kCenterStreamV4:
        case kCenterStream:     // its per-chunk column sums borrow W, which is not written before the stacked product
            return basd_teacher_center_stream(a->tok_ptrs, td, a->mix, L, G, a->t_sb, a->t_sn, a->t_sd, B, n, d_t, a->g0,
                                              a->g1, a->glam, a->omega_t, a->mu_t, a->tc, a->W, st);
        case kCenterMulti:
            return basd_teacher_center_multi(a->tok_ptrs, td, a->mix, L, G, a->t_sb, a->t_sn, a->t_sd, B, n, d_t, a->g0,
                                             a->g1, a->glam, a->omega_t, a->mu_t, a->tc, st);
        case kCenterPerGroup:
            for (int g = 0; g < G; ++g)
                BASD_TRY(basd_teacher_center(a->tok_ptrs, td, a->mix + (long)g * L, L, a->t_sb, a->t_sn, a->t_sd, B, n, d_t,
                                             a->g0, a->g1, a->glam, a->omega_t + (long)g * B * n,
                                             a->mu_t + (long)g * B * d_t, a->tc + (long)g * B * n * d_t, st));
            return BASD_OK;
        default:
            return BASD_EUNSUPPORTED;
    }
}
// The fp64 Gram of the centred teacher into g_b (G*B, n, n), split over the contraction where the plan says so.
static int teacher_gram(const BasdProcrustesArgs* a, const basd::plan::ProcrustesPlan& p, double* g_b, hipStream_t st) {
    const int n = (int)a->n, d_t = (int)a->d_t, GB = (int)a->G * (int)a->B;
    if (p.gram_split)
        return basd_gram_f64_split(a->tc, (long)n * d_t, n, d_t, GB, (int)a->g_splits, a->g_slabs, g_b, st);
    return basd_gram_f64(a->tc, (long)n * d_t, n, d_t, GB, g_b, (long)n * n, st);
}

// relational.py:22-50 for all extraction layers against the (mixed) teacher, forward and -- optionally -- the student
// gradients for given upstream gradients; see BasdProcrustesArgs in include/basd_hip.h.  The routes are those of the
// plan: where it names one of several entry points, that one is called and a refusal is returned as the error it is,
// never answered with another route.  The stages with a single entry point (Grams, Cholesky, finalize) are simply
// called: past their bounds they refuse for themselves, from the predicates the plan's status is made of, and the
// call ends there as it does at a stage without a route.
// teacher_given (basd_procrustes_forward_cached): omega, omega_t and the teacher slot of g_all are inputs; the token
// weights, the centring and the teacher Gram are not queued and tok_ptrs, attn_ptrs, mix, mu_t, tc, g_slabs not read.
static int procrustes_call(const BasdProcrustesArgs* a, hipStream_t st, bool teacher_given) {
    using namespace basd::plan;
    BASD_CHECK_ARG(a && a->student_ptrs);
    if (teacher_given) BASD_CHECK_ARG(a->omega && a->omega_t && a->g_all);
    else BASD_CHECK_ARG(a->tok_ptrs && a->attn_ptrs && a->mix);
    ProcrustesPlan p;
    BASD_TRY(procrustes_plan(a, g_transposed_cores, g_finish_fused, &p, teacher_given));
    const int E = (int)a->E, G = (int)a->G, B = (int)a->B, n_s = (int)a->n_s;
    const int d_s = (int)a->d_s, n = (int)a->n;
    const int sd = (int)a->s_dtype;
    // teacher side (teacher_given: kCenterGiven, nothing is queued)
    if (!teacher_given) BASD_TRY(teacher_weights_and_centring(a, p, st));
    // student side
    const long om_stride = G == 1 ? 0 : (long)B * n_s;
    if (p.project == kProjectNone) return p.status();
    if (p.project == kProjectMulti) {
        BASD_TRY(basd_student_project_multi(a->student_ptrs, sd, a->s_sb, a->s_sn, E, B, n_s, n, d_s, (int)a->s_aligned,
                                            a->omega, om_stride, a->tap0, a->tap1, a->lam, a->range0, a->range1, a->mu_s,
                                            a->tr_part, a->a_prime, st));
    } else {
        for (int e = 0; e < E; ++e)
            BASD_TRY(basd_student_project(a->student_host_ptrs[e], sd, a->s_sb, a->s_sn, B, n_s, n, d_s,
                                          a->omega + e * om_stride, a->tap0, a->tap1, a->lam, a->range0, a->range1,
                                          a->mu_s + (long)e * B * d_s, a->tr_part + (long)e * B * p.slabs,
                                          a->a_prime + (long)e * B * n * d_s, st));
    }
    // fp64 Grams on the core grid, Cholesky factors, product, SVD, per-sample terms
    const long nn = (long)n * n;
    const int EB = E * B, GB = G * B;
    double* g_b = a->g_all + (long)EB * nn;
    double* l_b = a->l_all + (long)EB * nn;
    BASD_TRY(basd_gram_f64(a->a_prime, (long)n * d_s, n, d_s, EB, a->g_all, nn, st));
    // (teacher_given: g_b is the caller's (basd_teacher_cache_load), factored below with the student Grams all the same)
    if (!teacher_given) BASD_TRY(teacher_gram(a, p, g_b, st));
    BASD_TRY(basd_chol_f64(a->g_all, nn, n, EB + GB, a->l_all, nn, st));
    if (p.cores == kCoresTransposed) {
        BASD_TRY(basd_stack_product_t(a->l_all, l_b, nn, n, EB, GB, a->W, 2 * nn, st));
        if (p.rebuild_usigma) BASD_TRY(basd_ustack_stash(a->W, 2 * nn, n, EB, a->w_stack, 2 * nn, st));
        BASD_TRY(basd_jacobi_onesided(a->W, 2 * nn, n, n, n, EB, nullptr, a->sigma, n, (int)a->max_sweeps, 0.f,
                                      a->jflags, a->sweeps, st));
    } else {
        BASD_TRY(basd_stack_product(a->l_all, l_b, nn, n, EB, GB, a->W, 2 * nn, st));
        int rc = BASD_EUNSUPPORTED;
        if (p.svd == kSvdTwoPass)       // the one route that is tried: see Svd
            rc = basd_jacobi_stacked_twopass(a->W, 2 * nn, n, EB, a->sigma, n, (int)a->max_sweeps, 0.f, a->jac_ws,
                                             a->sweeps, st);
        if (rc == BASD_EUNSUPPORTED)
            rc = basd_jacobi_onesided(a->W, 2 * nn, n, 2 * n, n, EB, nullptr, a->sigma, n, (int)a->max_sweeps, 0.f,
                                      a->jflags, a->sweeps, st);
        if (rc != BASD_OK) return rc;
    }
    if (p.finish == kFinishTransposed) {
        // cores of up to 64 tokens: the per-sample terms and K' in one launch, same bits (see the kernel)
        BASD_TRY(basd_procrustes_finish_transposed(a->W, 2 * nn, a->sigma, n, n_s, EB, GB, g_b, nn, a->omega, a->tap0,
                                                   a->tap1, a->lam, a->tr_part, p.slabs, a->tr_s, a->tr_t, a->nuc,
                                                   a->loss_b, l_b, nn, GB, a->k_prime, st));
    } else {
        // behind the transposed cores K' = Y Sigma^+ Y^T needs Y = L_b V first: not in finalize's reach
        BASD_TRY(basd_procrustes_finalize(a->W, 2 * nn, a->sigma, n, n_s, EB, GB, g_b, nn, a->omega, a->tap0, a->tap1,
                                          a->lam, a->tr_part, p.slabs, a->tr_s, a->tr_t, a->nuc, a->loss_b,
                                          p.cores == kCoresTransposed ? nullptr : a->k_prime, st));
        if (p.finish == kFinalizeKprimeT)
            BASD_TRY(basd_kprime_from_transposed(a->W, 2 * nn, a->sigma, n, EB, l_b, nn, GB, a->W + nn, 2 * nn,
                                                 a->k_prime, st));
    }
    if (p.rebuild_usigma) {
        BASD_CHECK_ARG(a->sigma_u != nullptr);
        // (scratch: the z region behind X, free again once K' has been formed)
        BASD_TRY(basd_ustack_from_transposed(a->W, 2 * nn, a->sigma, n, EB, a->w_stack, 2 * nn, a->W + nn, 2 * nn,
                                             a->sigma_u, (int)a->max_sweeps, a->jflags, st));
    }
    // combined.py:76-85: the UW-SO weights and the total, on the device (the student gradients below are then final)
    const float* grad_layers = a->grad_layers;
    if (a->uw_ce) {
        BASD_CHECK_ARG(a->uw_out != nullptr);
        basd::uwso_combine_kernel<<<1, 256, 0, st>>>(a->uw_ce, a->loss_b, E, B, a->uw_out);
        grad_layers = a->uw_out + 4;
    }
    // student gradients for the upstream gradients grad_layers (E floats on the device): H = K' A', then one pass
    if (p.grad != kGradNone) BASD_CHECK_ARG(a->k_prime && a->h && grad_layers);
    if (p.grad == kGradFused) {
        BASD_TRY(basd_student_grad_fused(a->student_ptrs, sd, a->s_sb, a->s_sn, E, B, n_s, n, d_s, (int)a->s_aligned,
                                         a->omega, om_stride, a->mu_s, a->k_prime, a->a_prime, a->tap0, a->tap1, a->lam,
                                         grad_layers, 2.0f / (float)B, a->dx, st));
    } else if (p.grad == kGradGemmMulti) {
        BASD_TRY(basd_gemm_tn(a->k_prime, a->a_prime, BASD_DTYPE_F32, 0, n, 1, nn, 0, d_s, 1, (long)n * d_s, 1 << 30, n,
                              n, d_s, EB, nullptr, nullptr, 1, nullptr, a->h, d_s, (long)n * d_s, 1.f, st));
        BASD_TRY(basd_student_grad_multi(a->student_ptrs, sd, a->s_sb, a->s_sn, E, B, n_s, n, d_s, a->omega, om_stride,
                                         a->mu_s, a->h, a->tap0, a->tap1, a->lam, grad_layers, 2.0f / (float)B, a->dx,
                                         nullptr, nullptr, st));
    }
    return BASD_OK;
}
int basd_procrustes_forward_fused(const BasdProcrustesArgs* a, hipStream_t st) { return procrustes_call(a, st, false); }
int basd_procrustes_forward_cached(const BasdProcrustesArgs* a, hipStream_t st) { return procrustes_call(a, st, true); }
// The teacher half alone, for ONE teacher layer: see include/basd_hip.h.  Nothing of the student is read or queued.
int basd_procrustes_teacher_side(const BasdProcrustesArgs* a, hipStream_t st) {
    using namespace basd::plan;
    BASD_CHECK_ARG(a && a->tok_ptrs && a->attn_ptrs && a->mix && a->omega && a->omega_t && a->mu_t && a->tc && a->g_all);
    ProcrustesPlan p;
    BASD_TRY(teacher_side_plan(a, &p));
    if (p.teacher_status() != BASD_OK) return p.teacher_status();       // before anything is queued
    BASD_CHECK_ARG(!p.gram_split || a->g_splits <= 64);
    BASD_TRY(teacher_weights_and_centring(a, p, st));
    return teacher_gram(a, p, a->g_all, st);
}

// Events for ordering two streams from inside a library call (see basd_tridiag_ranked's mid_event).
int basd_event_create(void** out) {
    BASD_CHECK_ARG(out);
    hipError_t e = hipEventCreateWithFlags((hipEvent_t*)out, hipEventDisableTiming);
    return e == hipSuccess ? BASD_OK : (int)e;
}
int basd_event_destroy(void* ev) {
    hipError_t e = hipEventDestroy((hipEvent_t)ev);
    return e == hipSuccess ? BASD_OK : (int)e;
}
int basd_stream_wait_event(hipStream_t stream, void* ev) {
    BASD_CHECK_ARG(ev);
    hipError_t e = hipStreamWaitEvent(stream, (hipEvent_t)ev, 0);
    return e == hipSuccess ? BASD_OK : (int)e;
}

}  // extern "C"
