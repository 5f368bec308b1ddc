// Which kernels one tridiagonal factorisation takes and how they are launched (tridiag_plan), the layout of its
// workspace, and the tiles of the vector stages of tridiag.hip -- each decision written once.  Host only: no HIP call is
// made and no pointer is dereferenced.  tridiag_impl issues the launches a plan names; basd_tridiag_workspace_bytes,
// basd_tridiag_plan_query and the selector chain's read-back of the status words (chain.hip) answer from the same code.
#pragma once
#include "basd_common.h"

namespace basd {

// shapes shared by the kernels of tridiag.hip and the plans below
constexpr int TRI_BLK = 32;            // shared stage: rows per ownership block (4 groups)
constexpr int TRI_TAIL_MAX = 256;      // order of the register-resident trailing block of tridiag_tail2_kernel
constexpr int PK_WAVES = 8, PK_NMAX = 384;   // tridiag_packed_kernel: waves per matrix, largest order

namespace plan {

constexpr int TRI_NMAX = 4096;         // 12 bits of step in the granule tags of the shared stage
constexpr int TRI_BUDGET_CAP = 128;    // workgroups of one shared-stage launch: see tridiag_resident_budget

// Hooks of basd_tridiag_tuning (their load-time values come from the environment: tridiag.hip).
//   tail  1 (default): orders 257..384 whole in tridiag_packed_kernel (one CU's registers, upper triangle), other orders
//         shared stage + tridiag_tail2_kernel; 3: shared stage + tail2 for every order (the round-2 path); 0: the whole
//         factorisation in the shared stage (the round-1 path).  Tests compare all of them.
struct TridiagTuning {
    int members = 0, pad = -1, lag = -1, threads = 0, tail = 1;
};
inline bool tail_is_valid(int tail) { return tail == 0 || tail == 1 || tail == 3; }

// per matrix: 2 parities x n granules of 16 bytes, then the pending (v, w) handed to the tail stage; at the very end
// the status word and 7 words of give-up trace
struct TridiagWorkspace {
    long granule_bytes, pend_off, status_off, bytes;
};
inline TridiagWorkspace tridiag_workspace(int n, int batch) {
    const long gran = (long)batch * 2 * n * 16, pend = (long)batch * 2 * n * 4;
    return {gran, gran, gran + pend, gran + pend + 32};
}

enum Front { kFrontNone = 0, kFrontShared };                       // tridiag_kernel on steps [0, j_stop)
enum Back { kBackNone = 0, kBackTail2, kBackPacked };              // tridiag_tail2_kernel / tridiag_packed_kernel
enum Variant { kScalar = 0, kVec, kVecFull };                      // tridiag_kernel<VEC, FULL>
enum Ranks { kRanksNone = 0, kRanksInBack, kRanksSeparate };       // separate: one tridiag_mp_rank_kernel launch

struct TridiagPlan {
    int status;                 // BASD_OK, or what the entry point returns instead of launching anything
    int front, back, j_stop;    // the back stage takes steps [j_stop, n - 1)
    int variant, members, batch_pad, grid, threads;      // shared stage (front != kFrontNone)
    long lds;
    bool memset_status;         // no shared stage writes the status words: they are cleared by a 32-byte fill
    int ranks;
    bool gated_ok;              // basd_tridiag_ranked_gated takes the shape: only a one-kernel factorisation can be queued early
    TridiagWorkspace ws;
};

inline int tridiag_status(int n, int batch) {
    if (n < 2 || batch < 1) return BASD_EINVAL;
    return n > TRI_NMAX ? BASD_EUNSUPPORTED : BASD_OK;
}
inline int tridiag_back(int n, int tail) {
    if (tail == 0) return kBackNone;
    return tail == 1 && n > TRI_TAIL_MAX && n <= PK_NMAX ? kBackPacked : kBackTail2;
}
inline int tridiag_j_stop(int n, int tail) {
    const int back = tridiag_back(n, tail);
    return back == kBackNone ? n - 1 : back == kBackTail2 && n > TRI_TAIL_MAX ? n - TRI_TAIL_MAX : 0;
}
// Only a plan with a shared stage reads `resident_budget`: the caller need not find one out for the others.
inline bool tridiag_needs_budget(int n, int batch, int tail) {
    return tridiag_status(n, batch) == BASD_OK && tridiag_j_stop(n, tail) > 0;
}

// quads: the matrices can be read as 16-byte quads (16-byte aligned base, batch stride a multiple of 4 floats).
// resident_budget: workgroups of the shared stage that may spin on each other (tridiag_resident_budget).
inline TridiagPlan tridiag_plan(int n, int batch, bool quads, bool ranked, bool gated, const TridiagTuning& t,
                                int resident_budget) {
    TridiagPlan p = {};
    p.status = tridiag_status(n, batch);
    if (p.status != BASD_OK) return p;
    p.ws = tridiag_workspace(n, batch);
    p.back = tridiag_back(n, t.tail);
    p.gated_ok = p.back == kBackPacked;
    if (gated && !p.gated_ok) p.status = BASD_EUNSUPPORTED;
    p.j_stop = tridiag_j_stop(n, t.tail);
    p.memset_status = p.j_stop == 0;
    if (p.j_stop > 0) {
        p.front = kFrontShared;
        p.variant = !(quads && n % 4 == 0) ? kScalar : n % 8 == 0 ? kVecFull : kVec;
        // one member per 32-row block, at most 16, fewer while the launch would not be resident as a whole
        const int nblk = (n + TRI_BLK - 1) / TRI_BLK;
        int P = t.members > 0 ? t.members : nblk;
        if (P > 16) P = 16;
        while (P > 1 && P * batch > resident_budget) --P;
        if (P > nblk) P = nblk;
        p.members = P < 1 ? 1 : P;
        // workgroup ids that differ by a multiple of 8 are dealt to one XCD: the members of a matrix share an L2
        p.batch_pad = t.pad >= 0 ? batch + t.pad : p.members > 1 ? (batch + 7) & ~7 : batch;
        p.grid = p.members * p.batch_pad;
        p.threads = t.threads > 0 ? t.threads : 1024;      // why never fewer in production: see tridiag_impl
        p.lds = (long)sizeof(float) * 9 * n;
    }
    // the workgroup that finishes a factorisation stages the tridiagonal in LDS for the ranks: 2 n floats in 8 KB
    if (ranked) p.ranks = p.back != kBackNone && 2 * n <= 8 * TRI_TAIL_MAX ? kRanksInBack : kRanksSeparate;
    return p;
}

// ---- vector stages ----------------------------------------------------------------------------------------------
// tridiag_invit_kernel / tridiag_shifted_solve_kernel: one wave works on vpw vectors at once, six arrays of n floats
// each in LDS ([array][element][vector]).  vpw == 0: not one vector fits.
struct SolveTile {
    int vpw;
    size_t lds;
};
inline SolveTile solve_tile(int n) {
    int vpw = (int)((144 * 1024) / (6 * sizeof(float) * (size_t)n));
    if (vpw > 64) vpw = 64;
    return {vpw, sizeof(float) * 6 * (size_t)n * vpw};
}
// backtransform_kernel<EPL>: elements of a vector per lane (64 lanes per vector).  0: no route for the order.
inline int backtransform_epl(int n) { return n <= 192 ? 3 : n <= 384 ? 6 : n <= 768 ? 12 : n <= 1024 ? 16 : 0; }

}  // namespace plan
}  // namespace basd
