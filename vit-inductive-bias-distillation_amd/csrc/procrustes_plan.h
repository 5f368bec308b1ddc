// Which kernels one Procrustes call takes: the applicability predicates of the per-kernel entry points of
// procrustes.hip, each written once, and procrustes_plan(), which chains them into the routes of
// basd_procrustes_forward_fused (fused.hip).  Host only: no HIP call is made and no pointer is dereferenced (pointers
// are tested for presence and 16-byte alignment).  The entry points answer BASD_EUNSUPPORTED from the same predicates,
// so the launcher never has to try one to learn whether it applies.
#pragma once
#include "basd_common.h"
#include "../../include/basd_hip.h"

namespace basd {

// tile shapes shared by the kernels of procrustes.hip and the LDS sizes below
constexpr int SP_W = 32;                              // student_project_v4_kernel: slab width in features
constexpr int SP_W1 = 64;                             // student_project_kernel (per layer): slab width
constexpr int TCM_W = 16, TCM_G = 4;                  // teacher_center_multi_kernel: slab width, groups per pass
constexpr int TCS_ROWS = 16;                          // teacher_mix_stream*_kernel: token rows per chunk
constexpr int G64_BK = 32, G64_LD = 36, G64_TPW = 8;  // gram_f64_kernel
constexpr int CB_NB = 16, CB_KC = 64, CB_MAXR = 16;   // chol_f64_blocked_kernel
constexpr int SG_W = 64;                              // student_grad_fused_kernel: slab width in features
constexpr int SG_LD = SG_W + 4;                       //   row stride of the H slab in LDS

namespace plan {

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// rows of a (B, n, D) token tensor with unit feature stride can be read as 16-byte quads from a 16-byte aligned base
// (4 fp32 or -- two quads per load -- 8 bf16 features)
inline bool rows_are_quads(int dtype, long sb, long sn, int D) {
    const int esz = dtype == BASD_DTYPE_F32 ? 4 : 2;
    return D % 4 == 0 && (sb * esz) % 16 == 0 && (sn * esz) % 16 == 0 && (esz == 4 || D % 8 == 0);
}

// ---- teacher centring -------------------------------------------------------------------------------------------
inline size_t center_lds(int n) { return sizeof(float) * ((size_t)n * 65 + n + 64); }
inline bool center_fits(int n) { return center_lds(n) <= 150 * 1024; }
inline size_t center_multi_lds(int G, int n) {
    return sizeof(float) * ((size_t)G * n * (TCM_W + 1) + (size_t)G * n + (size_t)G * TCM_W);
}
inline bool center_multi_applies(int G, int n) { return G <= TCM_G && center_multi_lds(G, n) <= 150 * 1024; }
inline int stream_chunks(int n) { return (n + TCS_ROWS - 1) / TCS_ROWS; }
inline long stream_scratch_floats(int G, int B, int n, int D) { return (long)stream_chunks(n) * G * B * D; }
inline bool stream_applies(int G, long sd, int B) { return G <= TCM_G && sd == 1 && B <= 65535 && (long)G * B <= 65535; }
// fp32 tokens on the teacher's own grid whose rows, like the outputs, are 16-byte aligned: four features per thread
inline bool stream_v4_applies(int dtype, bool gathered, long sb, long sn, int D, const void* tc, const void* scratch) {
    return dtype == BASD_DTYPE_F32 && !gathered && D % 4 == 0 && sb % 4 == 0 && sn % 4 == 0 && aligned16(tc) &&
           aligned16(scratch);
}

// ---- student projection -----------------------------------------------------------------------------------------
inline size_t project_lds(int n_s) { return sizeof(float) * (size_t)n_s; }
inline size_t project_multi_lds(int n_s) { return sizeof(float) * ((size_t)n_s * SP_W + 5 * (size_t)n_s); }
inline bool project_multi_applies(int ptrs_aligned, int dtype, long sb, long sn, int D, int n_s) {
    return ptrs_aligned && rows_are_quads(dtype, sb, sn, D) && project_multi_lds(n_s) <= 96 * 1024;
}
// partial traces per sample: one per slab of `width` features
inline int trace_slabs(int D, int width) { return (D + width - 1) / width; }

// ---- Grams, Cholesky, cores -------------------------------------------------------------------------------------
inline size_t gram_lds(int n) { return sizeof(float) * (size_t)((n + 15) / 16) * 16 * G64_LD; }
inline bool gram_fits(int n) { return gram_lds(n) <= 156 * 1024; }
inline size_t chol_lds(int n) { return sizeof(double) * ((size_t)n * (n + 1) / 2 + n); }
inline size_t chol_blocked_lds(int n) { return sizeof(double) * ((size_t)n * CB_NB + (size_t)CB_NB * (CB_KC + 1)); }
inline bool chol_in_lds(int n) { return chol_lds(n) <= 158 * 1024; }
inline bool chol_blocked_fits(int n) { return n <= 64 * CB_MAXR; }
// the stacked cores of this many batched matrices occupy W; the stream centring borrows it before it is written
inline long core_floats(int E, int B, int n) { return (long)E * B * 2 * n * n; }
// transposed cores where the hook and the batch allow them (hook: basd_procrustes_tuning)
inline bool transposed_cores_wanted(int hook, int EB) { return hook == 2 || (hook == 1 && EB >= 128); }

// ---- finish -----------------------------------------------------------------------------------------------------
inline size_t finalize_lds(int n, bool k_prime) { return sizeof(float) * ((size_t)n + (k_prime ? (size_t)n * n : 0)); }
inline bool finalize_fits(size_t lds) { return lds <= 156 * 1024; }
inline bool small_core(int n) { return n <= 64; }        // the fused finish and the fused student gradient
inline bool finish_transposed_applies(int n, int batch) { return small_core(n) && batch <= 65535; }
inline size_t finish_transposed_lds(int n) {
    const int nq = (n + 3) / 4, np = 4 * nq, ld = (nq & 1) ? np : np + 4;
    return sizeof(float) * (size_t)(3 * np * ld + np);      // <= 52480 bytes
}

// ---- student gradient -------------------------------------------------------------------------------------------
inline size_t grad_fused_lds(int n_t) { return sizeof(float) * (size_t)n_t * (SG_W + SG_LD); }
inline bool grad_fused_applies(int ptrs_aligned, int dtype, long sb, long sn, int D, int n_t, const void* a_prime,
                               const void* mu, const void* dx) {
    return ptrs_aligned && small_core(n_t) && n_t >= 4 && rows_are_quads(dtype, sb, sn, D) && aligned16(a_prime) &&
           aligned16(mu) && aligned16(dx);
}

// ---- the plan ---------------------------------------------------------------------------------------------------
// kCenterGiven: the teacher side is an input of the call (basd_procrustes_forward_cached), nothing is centred
enum Center { kCenterNone = 0, kCenterStreamV4, kCenterStream, kCenterMulti, kCenterPerGroup, kCenterGiven };
enum Project { kProjectNone = 0, kProjectMulti, kProjectPerLayer };
enum Chol { kCholNone = 0, kCholLds, kCholBlocked };
enum Cores { kCoresTransposed = 1, kCoresStacked };
// kSvdTwoPass: basd_jacobi_stacked_twopass with the offered workspace, basd_jacobi_onesided where it answers that it
// does not cover the order (jacobi.hip has no exact query for that: the one try-and-fall-back left in the launcher)
enum Svd { kSvdTransposed = 1, kSvdTwoPass, kSvdStacked };
enum Finish { kFinishNone = 0, kFinishTransposed, kFinalizeKprimeT, kFinalize, kFinalizeTiledKprime };
enum Grad { kGradNone = 0, kGradFused, kGradGemmMulti };
enum USigma { kUSigmaInW = 1, kUSigmaInWStack };

struct ProcrustesPlan {
    int center, project, slab_width, slabs, gram_split, chol, cores, svd, finish, rebuild_usigma, grad, usigma_in;
    long tr_part_floats, w_borrow_floats;                  // scratch the routes need from the caller
    long lds_center, lds_project, lds_gram, lds_chol, lds_finish, lds_grad;   // dynamic LDS bytes of the named kernels
    // what a call with this plan returns where it reaches a stage that has no route
    int status() const {
        if (project == kProjectNone) return BASD_EINVAL;
        const bool routed = center != kCenterNone && lds_gram >= 0 && chol != kCholNone && finish != kFinishNone;
        return routed ? BASD_OK : BASD_EUNSUPPORTED;
    }
    // the same for basd_procrustes_teacher_side, which ends behind the teacher Gram: asked BEFORE anything is queued
    int teacher_status() const { return center != kCenterNone && lds_gram >= 0 ? BASD_OK : BASD_EUNSUPPORTED; }
};
constexpr int kPlanFields = 20;

// The teacher half of a plan, the one statement of it for the uncached call and for basd_procrustes_teacher_side: the
// centring route with what it borrows, whether the teacher Gram is split, the Gram's LDS (-1: past LDS).
inline void plan_teacher_half(const BasdProcrustesArgs* a, ProcrustesPlan* p) {
    const int E = (int)a->E, L = (int)a->L, G = (int)a->G, B = (int)a->B, d_t = (int)a->d_t, n = (int)a->n;
    // all groups in one pass over the teacher layers where that applies
    const long borrow = stream_scratch_floats(G, B, n, d_t);
    if (G > 1 && L >= 4 && borrow <= core_floats(E, B, n) && stream_applies(G, a->t_sd, B)) {
        p->center = stream_v4_applies((int)a->t_dtype, a->g0 != nullptr, a->t_sb, a->t_sn, d_t, a->tc, a->W)
                        ? kCenterStreamV4 : kCenterStream;
        p->w_borrow_floats = borrow;
    } else if (G > 1 && center_multi_applies(G, n)) {
        p->center = kCenterMulti;
        p->lds_center = (long)center_multi_lds(G, n);
    } else if (center_fits(n)) {
        p->center = kCenterPerGroup;
        p->lds_center = (long)center_lds(n);
    }
    p->gram_split = a->g_slabs && a->g_splits > 1;
    p->lds_gram = gram_fits(n) ? (long)gram_lds(n) : -1;
}

// The plan of basd_procrustes_teacher_side: the teacher half for ONE layer and ONE group, every student-side stage
// "none" (0).  The student's fields of the block (E, d_s, the student pointers and layout) are not read.  More than one
// layer or group: no route (teacher_status() is BASD_EUNSUPPORTED), as for a core grid past the centring kernel's LDS.
inline int teacher_side_plan(const BasdProcrustesArgs* a, ProcrustesPlan* out) {
    BASD_CHECK_ARG(a && out);
    const int L = (int)a->L, G = (int)a->G, B = (int)a->B, n_s = (int)a->n_s, n_t = (int)a->n_t, n = (int)a->n;
    BASD_CHECK_ARG(L > 0 && G > 0 && B > 0 && n > 0 && n == (n_s < n_t ? n_s : n_t) && a->d_t > 0);
    BASD_CHECK_ARG(B <= 65535);               // samples index grid.y of the centring kernel
    ProcrustesPlan p = {};
    if (L == 1 && G == 1) plan_teacher_half(a, &p);
    *out = p;
    return BASD_OK;
}

// Shapes and presence of the optional pointers are read from the call's own argument block; transposed_hook and
// finish_hook are the settings of basd_procrustes_tuning / basd_procrustes_finish_tuning.  teacher_given: the plan of
// basd_procrustes_forward_cached (G == 1 only) -- no centring, no teacher Gram; every later stage as without it.
inline int procrustes_plan(const BasdProcrustesArgs* a, int transposed_hook, int finish_hook, ProcrustesPlan* out,
                           bool teacher_given = false) {
    BASD_CHECK_ARG(a && out);
    const int E = (int)a->E, L = (int)a->L, G = (int)a->G, B = (int)a->B, n_s = (int)a->n_s, n_t = (int)a->n_t;
    const int d_s = (int)a->d_s, d_t = (int)a->d_t, n = (int)a->n;
    BASD_CHECK_ARG(E > 0 && L > 0 && (G == 1 || G == E) && B > 0 && n == (n_s < n_t ? n_s : n_t));
    BASD_CHECK_ARG(n > 0 && d_s > 0 && d_t > 0);
    BASD_CHECK_ARG(!teacher_given || G == 1);
    const int EB = E * B;
    ProcrustesPlan p = {};

    // teacher side (the student Grams share the Gram kernel, hence its LDS either way)
    if (teacher_given) {
        p.center = kCenterGiven;
        p.lds_gram = gram_fits(n) ? (long)gram_lds(n) : -1;
    } else {
        plan_teacher_half(a, &p);
    }

    // student side: all layers in one launch where the vectorised kernel applies
    // (layers and samples index grid.z / grid.y of the student kernels: past 65535 of either there is no projection,
    // and the call ends there with BASD_EINVAL, behind the teacher-side launches as it always has)
    if (E <= 65535 && B <= 65535) {
        const bool multi = project_multi_applies((int)a->s_aligned, (int)a->s_dtype, a->s_sb, a->s_sn, d_s, n_s);
        p.project = multi ? kProjectMulti : kProjectPerLayer;
        p.slab_width = multi ? SP_W : SP_W1;
        p.slabs = trace_slabs(d_s, p.slab_width);
        p.tr_part_floats = (long)EB * p.slabs;
        p.lds_project = (long)(multi ? project_multi_lds(n_s) : project_lds(n_s));
    }

    p.chol = chol_in_lds(n) ? kCholLds : chol_blocked_fits(n) ? kCholBlocked : kCholNone;
    p.lds_chol = (long)(p.chol == kCholLds ? chol_lds(n) : chol_blocked_lds(n));

    // Cores that the plain 4-lane LDS solver takes: the Jacobi runs on M^T alone -- its columns come out as V Sigma --
    // and Y = L_b V is formed when K' is (half the rows per pair-step, no two-pass / block solver at 144 tokens).
    // With gradients through the mixing weights (raw set) the backward reads U Sigma, the top half of the stacked
    // cores: it is rebuilt from the transposed route's Z afterwards, which needs w_stack.
    const bool transposed = (a->raw == nullptr || a->w_stack != nullptr) && EB <= 65535 && basd_jacobi_plain4_fits(n) &&
                            transposed_cores_wanted(transposed_hook, EB);
    if (transposed) {
        p.cores = kCoresTransposed;
        p.svd = kSvdTransposed;
        p.finish = !a->k_prime ? kFinalize
                   : finish_hook && finish_transposed_applies(n, EB) ? kFinishTransposed : kFinalizeKprimeT;
        p.lds_finish = (long)(p.finish == kFinishTransposed ? finish_transposed_lds(n) : finalize_lds(n, false));
        p.rebuild_usigma = a->raw != nullptr;
    } else {
        p.cores = kCoresStacked;
        p.svd = a->jac_ws ? kSvdTwoPass : kSvdStacked;
        const bool tiled = !finalize_fits(finalize_lds(n, a->k_prime != nullptr));    // K' past LDS: a tiled kernel
        p.finish = tiled ? kFinalizeTiledKprime : kFinalize;
        p.lds_finish = (long)finalize_lds(n, a->k_prime != nullptr && !tiled);
    }
    if (!finalize_fits((size_t)p.lds_finish)) p.finish = kFinishNone;
    p.usigma_in = p.rebuild_usigma ? kUSigmaInWStack : kUSigmaInW;

    if (a->dx) {
        const bool fused = grad_fused_applies((int)a->s_aligned, (int)a->s_dtype, a->s_sb, a->s_sn, d_s, n, a->a_prime,
                                              a->mu_s, a->dx);
        p.grad = fused ? kGradFused : kGradGemmMulti;
        p.lds_grad = fused ? (long)grad_fused_lds(n) : 0;
    }
    *out = p;
    return BASD_OK;
}

}  // namespace plan
}  // namespace basd
