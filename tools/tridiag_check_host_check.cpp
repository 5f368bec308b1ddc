// Host build of csrc/tridiag_check_core.h: the probe sums, the residual terms, the ratios and the verdict bits of the
// residual check, run serially on the CPU under the address and undefined-behaviour sanitizers.  No GPU, no HIP.
//
//   tridiag_check_host_check IN OUT
//
// IN : 4 x int64 (magic 0x54434B31, n, batch, thresholds given ? 1 : 0), 3 x fp32 thresholds, then per matrix fp32
//      a (n, n), d (n), e (n), tau (n), vh (n, n) -- a factorisation in the library's layout (row j of vh = reflector j).
// OUT: per matrix 2 x fp64 (tr A, |A|_F^2), 3 x fp64 ratios, int32 verdict bits, int32 0; then (batch, 2, n) fp32, the
//      probe rows x and y.
// The fp32 reflectors are applied here in fp64 and the result rounded to fp32 once, so that the numbers do not depend on
// the order of an fp32 dot product (the kernels' part of that is basd_tridiag_apply_q, which has its own tests).
// Every buffer is sized exactly, so an index past an end is a sanitizer report and a non-zero exit.
//
// Build: make -C vit-inductive-bias-distillation_amd/csrc tridiag_check_host_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../vit-inductive-bias-distillation_amd/csrc/tridiag_check_core.h"

namespace {

// x <- Q^T x = H_{n-2} ... H_0 x, H_j = I - tau_j v_j v_j^T, in fp64; rounded to fp32 at the end.
void apply_qt(const float* tau, const float* vh, int n, float* x32) {
    std::vector<double> x(x32, x32 + n);
    for (int j = 0; j + 1 < n; ++j) {
        if (tau[j] == 0.f) continue;
        const float* v = vh + (long)j * n;
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += (double)v[i] * x[i];
        s *= (double)tau[j];
        for (int i = 0; i < n; ++i) x[i] -= s * (double)v[i];
    }
    for (int i = 0; i < n; ++i) x32[i] = (float)x[i];
}

bool read_exact(std::FILE* f, void* dst, size_t bytes) { return std::fread(dst, 1, bytes, f) == bytes; }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int64_t head[4];
    float thr_in[3];
    if (!read_exact(in, head, sizeof head) || head[0] != 0x54434B31 || !read_exact(in, thr_in, sizeof thr_in)) return 3;
    const int n = (int)head[1], batch = (int)head[2];
    if (n < 1 || n > BASD_TRIDIAG_CHECK_MAX_N || batch < 1 || batch > 4096) return 3;
    const basd::TridiagProbeLayout layout = basd::tridiag_probe_layout(n, batch);
    if (layout.parts % 16 || layout.sums % 16 || layout.ctl % 16 || layout.bytes <= layout.ctl ||
        layout.n_parts * BASD_TRIDIAG_PROBE_ROWS < n)
        return 4;
    float thr[3];
    if (head[3]) std::memcpy(thr, thr_in, sizeof thr);
    else basd::tridiag_check_default_thresholds(n, thr);

    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    std::vector<float> rows((size_t)batch * 2 * n);
    for (int z = 0; z < batch; ++z) {
        std::vector<float> a((size_t)n * n), d(n), e(n), tau(n), vh((size_t)n * n), uv((size_t)2 * n);
        if (!read_exact(in, a.data(), a.size() * 4) || !read_exact(in, d.data(), d.size() * 4) ||
            !read_exact(in, e.data(), e.size() * 4) || !read_exact(in, tau.data(), tau.size() * 4) ||
            !read_exact(in, vh.data(), vh.size() * 4))
            return 3;
        double sums[2], rho[3];
        float* xy = rows.data() + (size_t)z * 2 * n;
        basd::tridiag_probe_serial(a.data(), n, (unsigned)z, xy, sums);
        std::memcpy(uv.data(), xy, uv.size() * 4);
        apply_qt(tau.data(), vh.data(), n, uv.data());
        apply_qt(tau.data(), vh.data(), n, uv.data() + n);
        const int32_t bits[2] = {basd::tridiag_check_serial(d.data(), e.data(), uv.data(), sums, n, thr, rho), 0};
        std::fwrite(sums, sizeof(double), 2, out);
        std::fwrite(rho, sizeof(double), 3, out);
        std::fwrite(bits, sizeof(int32_t), 2, out);
    }
    std::fwrite(rows.data(), sizeof(float), rows.size(), out);
    std::fclose(out);
    std::fclose(in);
    return 0;
}
