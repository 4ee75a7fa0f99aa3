/* The render kernels' exact-arithmetic primitives, run on their own: a stand-alone program that includes rt_device.h (the kernels'
 * text, not a copy), wraps every primitive in one small __global__ function and moves operands and results through binary files.
 * tests/test_gpu_device_math.py drives it on the device and compares with IEEE (numpy) references; tests/test_device_math_cases.py
 * uses the `host` mode, which makes no HIP call, to pin those references to rt_math.h's text on a machine without a GPU.
 *
 * Command line: one or more jobs, separated by "--":
 *     dev     NAME SHAPE IN OUT   run NAME on the device in launch shape SHAPE
 *     host    NAME IN OUT         run NAME on the host (HIP-free functions only)
 *     hostdev NAME IN OUT         run NAME on both, compare bit for bit here, print "hostdev NAME evals=N mismatches=M", write the
 *                                 device's results
 *     order   IN OUT              rt::order_kernel on a batch of cases
 * IN of a function with K operands is K columns of n float64 (n from the file's size); OUT is M columns of n 64-bit words (a float64
 * result as it is, a float32 result's 32 bits, a boolean 0/1; T names the words' types, 'd', 'f' and 'u').  float32 and unsigned
 * operands travel as float64 holding the value.
 * SHAPE: `full` (n a multiple of 64: every wave has all its lanes), `tail` (n = 37 mod 64: the last wave has 37), `odd` (the odd
 * lanes only, under a divergent if; the even lanes' results keep the sentinel).  The guards of normalize3 / renormalize_unit are
 * ballots over live lanes, so the shape is part of what is tested.
 * IN of `order`: int64 ncases, then per case int64 {nblocks, gshift, wshift, nvalid} and max(nvalid, 0) uint32 costs; OUT: per case
 * the 2 nblocks words of both permutations.
 * Every result buffer is filled with a sentinel first; every buffer is sized from the operand count and every count is checked
 * before a launch; every HIP call is checked and the first error ends the program (exit 2) before anything else is launched.
 * Built by python-ray-tracer_amd/csrc/Makefile (target `kat`) with the library's own HIPCC and FLAGS, a second time with
 * -DRT_FAST_NORMALIZE=0 -DRT_FAST_DIVSQRT=0 (the backend's own division and square root: device_math_kat_generic). */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../python-ray-tracer_amd/csrc/rt_device.h"

#pragma clang fp contract(off)

static constexpr uint64_t SENTINEL = 0xC0DEC0DEC0DEC0DEull;
static constexpr uint32_t SENTINEL32 = 0xC0DEC0DEu;
static constexpr long MAX_OPERANDS = 1l << 22;

#define CHECK_HIP(call)                                                                                               \
    do {                                                                                                              \
        const hipError_t e_ = (call);                                                                                 \
        if (e_ != hipSuccess) {                                                                                       \
            fprintf(stderr, "HIP error %d (%s) at %s:%d: %s\n", (int)e_, hipGetErrorString(e_), __FILE__, __LINE__, #call); \
            exit(2);                                                                                                  \
        }                                                                                                             \
    } while (0)

#define KAT_HD __host__ __device__ __forceinline__ static
#define KAT_D __device__ __forceinline__ static

KAT_HD uint64_t bits(double x) { uint64_t u; __builtin_memcpy(&u, &x, 8); return u; }
KAT_HD uint64_t bits(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return u; }
static bool is_nan64(uint64_t u) { return (u & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull; }
static bool is_nan32(uint64_t u) { return (u & 0x7FFFFFFFull) > 0x7F800000ull; }
KAT_HD unsigned u32(double x) { return (unsigned)x; }          // the operand files hold integers of [0, 2^32) there

// ---- the functions under test: K operands -> M result words ---------------------------------------------------------------
// HIP-free functions (rt_math.h, rt_cull.h, rt_facing.h): the same text on the host and on the device.
struct DivSeeded { static constexpr int K = 3, M = 1; static constexpr const char *T = "d"; static constexpr bool HOST = true;          // a, b, r = rcp(b)
    KAT_HD void f(const double *a, uint64_t *o) { o[0] = bits(rt::div_seeded(a[0], a[1], a[2])); } };
struct SqrtSeeded { static constexpr int K = 2, M = 3; static constexpr const char *T = "ddd"; static constexpr bool HOST = true;         // x, y = rsq(x)
    KAT_HD void f(const double *a, uint64_t *o)
    { const rt::SqrtIter s = rt::sqrt_iter(a[0], a[1]); o[0] = bits(rt::sqrt_seeded(a[0], a[1])); o[1] = bits(s.g); o[2] = bits(s.h); } };
struct Normalize3Seeded { static constexpr int K = 5, M = 3; static constexpr const char *T = "ddd"; static constexpr bool HOST = true;   // v, nn, y = rsq(nn)
    KAT_HD void f(const double *a, uint64_t *o)
    { const rt::V3 r = rt::normalize3_seeded(rt::V3{a[0], a[1], a[2]}, a[3], a[4]); o[0] = bits(r.x); o[1] = bits(r.y); o[2] = bits(r.z); } };
struct Normalize3Generic { static constexpr int K = 3, M = 4; static constexpr const char *T = "dddd"; static constexpr bool HOST = true;  // v; the fourth word is |v|² as normalize3 forms it
    KAT_HD void f(const double *a, uint64_t *o)
    {
        const rt::V3 v{a[0], a[1], a[2]}, r = rt::normalize3_generic(v);
        o[0] = bits(r.x); o[1] = bits(r.y); o[2] = bits(r.z); o[3] = bits(rt::dot3(v, v));
    } };
struct RenormalizeUnitFast { static constexpr int K = 4, M = 6; static constexpr const char *T = "dddddd"; static constexpr bool HOST = true;   // d, e; then unit_norm(e)
    KAT_HD void f(const double *a, uint64_t *o)
    {
        const rt::V3 r = rt::renormalize_unit_fast(rt::V3{a[0], a[1], a[2]}, a[3]);
        const rt::UnitNorm u = rt::unit_norm(a[3]);
        o[0] = bits(r.x); o[1] = bits(r.y); o[2] = bits(r.z); o[3] = bits(u.nrm); o[4] = bits(u.dl); o[5] = bits(u.y);
    } };
struct UnitWindow { static constexpr int K = 3, M = 2; static constexpr const char *T = "du"; static constexpr bool HOST = true;         // d -> unit_excess, outside_unit_window
    KAT_HD void f(const double *a, uint64_t *o)
    { const double e = rt::unit_excess(rt::V3{a[0], a[1], a[2]}); o[0] = bits(e); o[1] = rt::outside_unit_window(e) ? 1u : 0u; } };
struct AnchoredTau { static constexpr int K = 3, M = 1; static constexpr const char *T = "f"; static constexpr bool HOST = true;        // ll, r2, floor_anch (float32)
    KAT_HD void f(const double *a, uint64_t *o) { o[0] = bits(rt::anchored_tau(a[0], a[1], (float)a[2])); } };
struct CullAnchored { static constexpr int K = 7, M = 1; static constexpr const char *T = "u"; static constexpr bool HOST = true;       // entry (4 float32), R
    KAT_HD void f(const double *a, uint64_t *o)
    {
        const rt::f4 e = {(float)a[0], (float)a[1], (float)a[2], (float)a[3]};
        o[0] = rt::cull_anchored(e, rt::make_rayf_dir(rt::V3{a[4], a[5], a[6]})) ? 1u : 0u;
    } };
struct CullOrigin { static constexpr int K = 11, M = 3; static constexpr const char *T = "uff"; static constexpr bool HOST = true;        // sphere (4 float32), R, o, extent2 (float32)
    KAT_HD void f(const double *a, uint64_t *o)
    {
        const rt::f4 c = {(float)a[0], (float)a[1], (float)a[2], (float)a[3]};
        rt::RayF q = rt::make_rayf_dir(rt::V3{a[4], a[5], a[6]});
        rt::add_origin(q, rt::V3{a[7], a[8], a[9]}, (float)a[10]);
        o[0] = rt::cull_origin(c, q) ? 1u : 0u; o[1] = bits(q.mgq); o[2] = bits(q.esq);
    } };
struct Facing { static constexpr int K = 8, M = 4; static constexpr const char *T = "dduu"; static constexpr bool HOST = true;             // v, N, reach, lamb
    KAT_HD void f(const double *a, uint64_t *o)
    {
        const double tau = rt_facing_tau(a[6], a[7]);
        o[0] = bits(tau); o[1] = bits(rt_facing_u(a[0], a[1], a[2], a[3], a[4], a[5]));
        o[2] = (uint64_t)rt_facing_certified(a[0], a[1], a[2], a[3], a[4], a[5], tau);
        o[3] = (uint64_t)rt_facing_certified_lamb(a[0], a[1], a[2], a[3], a[4], a[5], tau, a[7]);
    } };
struct Hashes { static constexpr int K = 4, M = 8; static constexpr const char *T = "uuuuuudd"; static constexpr bool HOST = true;             // x, y, s, seed (unsigned)
    KAT_HD void f(const double *a, uint64_t *o)
    {
        const unsigned x = u32(a[0]), y = u32(a[1]), s = u32(a[2]), seed = u32(a[3]);
        o[0] = rt::hash_xy(seed, x, y); o[1] = rt::scatter_hash(x, s); o[2] = rt::jitter_hash(x, y, s, seed);
        o[3] = rt::scatter_key(x, y, s, seed); o[4] = rt::soft_key(x, y, s, seed); o[5] = rt::lens_key(x, y, s, seed);
        o[6] = bits(rt::hash_unit(x, s)); o[7] = bits(rt::hash_unit(rt::scatter_key(x, y, s, seed), y));
    } };
struct ClipColor { static constexpr int K = 1, M = 1; static constexpr const char *T = "u"; static constexpr bool HOST = true;
    KAT_HD void f(const double *a, uint64_t *o) { o[0] = rt::clip_color(a[0]); } };

// What only the device has (rt_device.h): the hardware's seeds, the four wrappers with their ballots, the cluster box test.
struct SeedRcp { static constexpr int K = 1, M = 1; static constexpr const char *T = "d"; static constexpr bool HOST = false;
    KAT_D void f(const double *a, uint64_t *o) { o[0] = bits(__builtin_amdgcn_rcp(a[0])); } };
struct SeedRsq { static constexpr int K = 1, M = 1; static constexpr const char *T = "d"; static constexpr bool HOST = false;
    KAT_D void f(const double *a, uint64_t *o) { o[0] = bits(__builtin_amdgcn_rsq(a[0])); } };
struct SeedRcpf { static constexpr int K = 1, M = 1; static constexpr const char *T = "f"; static constexpr bool HOST = false;          // a float32 operand
    KAT_D void f(const double *a, uint64_t *o) { o[0] = bits(__builtin_amdgcn_rcpf((float)a[0])); } };
struct Normalize3 { static constexpr int K = 3, M = 3; static constexpr const char *T = "ddd"; static constexpr bool HOST = false;
    KAT_D void f(const double *a, uint64_t *o)
    { const rt::V3 r = rt::normalize3(rt::V3{a[0], a[1], a[2]}); o[0] = bits(r.x); o[1] = bits(r.y); o[2] = bits(r.z); } };
struct RenormalizeUnit { static constexpr int K = 3, M = 3; static constexpr const char *T = "ddd"; static constexpr bool HOST = false;
    KAT_D void f(const double *a, uint64_t *o)
    { const rt::V3 r = rt::renormalize_unit(rt::V3{a[0], a[1], a[2]}); o[0] = bits(r.x); o[1] = bits(r.y); o[2] = bits(r.z); } };
struct DivInrange { static constexpr int K = 2, M = 1; static constexpr const char *T = "d"; static constexpr bool HOST = false;
    KAT_D void f(const double *a, uint64_t *o) { o[0] = bits(rt::div_inrange(a[0], a[1])); } };
struct SqrtInrange { static constexpr int K = 1, M = 1; static constexpr const char *T = "d"; static constexpr bool HOST = false;
    KAT_D void f(const double *a, uint64_t *o) { o[0] = bits(rt::sqrt_inrange(a[0])); } };
// make_raybox + box_open combined with RayBox::sane as lane_cluster_bits combines them: o, R (float64, as the kernel has them),
// extent2 and the box (float32).  Words: certificate (the box's spheres are skipped), box_open, sane.
struct RayBoxCert { static constexpr int K = 13, M = 3; static constexpr const char *T = "uuu"; static constexpr bool HOST = false;
    KAT_D void f(const double *a, uint64_t *o)
    {
        rt::RayF q = rt::make_rayf_dir(rt::V3{a[3], a[4], a[5]});
        rt::add_origin(q, rt::V3{a[0], a[1], a[2]}, (float)a[6]);
        const rt::RayBox rb = rt::make_raybox(q, (float)a[6]);
        const rt::f4 lo = {(float)a[7], (float)a[8], (float)a[9], 0.0f}, hi = {(float)a[10], (float)a[11], (float)a[12], 0.0f};
        const bool open = rt::box_open(lo, hi, rb) || !rb.sane;
        o[0] = open ? 0u : 1u; o[1] = rt::box_open(lo, hi, rb) ? 1u : 0u; o[2] = rb.sane ? 1u : 0u;
    } };

#define KAT_FUNCTIONS(X)                                                                                                      \
    X(DivSeeded, "div_seeded") X(SqrtSeeded, "sqrt_seeded") X(Normalize3Seeded, "normalize3_seeded")                          \
    X(Normalize3Generic, "normalize3_generic") X(RenormalizeUnitFast, "renormalize_unit_fast") X(UnitWindow, "unit_window")    \
    X(AnchoredTau, "anchored_tau") X(CullAnchored, "cull_anchored") X(CullOrigin, "cull_origin") X(Facing, "facing")           \
    X(Hashes, "hashes") X(ClipColor, "clip_color") X(SeedRcp, "seed_rcp") X(SeedRsq, "seed_rsq") X(SeedRcpf, "seed_rcpf")       \
    X(Normalize3, "normalize3") X(RenormalizeUnit, "renormalize_unit") X(DivInrange, "div_inrange") X(SqrtInrange, "sqrt_inrange") \
    X(RayBoxCert, "raybox")

// One thread per operand row, 256 per workgroup.  odd: the call sits under a divergent if that only the odd lanes take.
template <class F> __global__ __launch_bounds__(256) void eval_kernel(const double *__restrict__ in, uint64_t *__restrict__ out, long n, int odd)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (!odd || (threadIdx.x & 1)) {
        double a[F::K];
        uint64_t o[F::M];
        for (int c = 0; c < F::K; ++c) a[c] = in[(long)c * n + i];
        F::f(a, o);
        for (int c = 0; c < F::M; ++c) out[(long)c * n + i] = o[c];
    }
}

// ---- files ----------------------------------------------------------------------------------------------------------------
static std::vector<char> read_file(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(1); }
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<char> buf((size_t)(sz > 0 ? sz : 0));
    if (sz > 0 && fread(buf.data(), 1, (size_t)sz, f) != (size_t)sz) { fprintf(stderr, "short read of %s\n", path); exit(1); }
    fclose(f);
    return buf;
}
static void write_file(const char *path, const void *p, size_t bytes)
{
    FILE *f = fopen(path, "wb");
    if (!f || (bytes && fwrite(p, 1, bytes, f) != bytes) || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", path); exit(1); }
}
static long operand_rows(const std::vector<char> &buf, int K, const char *path)
{
    const size_t row = (size_t)K * sizeof(double);
    if (buf.empty() || buf.size() % row != 0 || (long)(buf.size() / row) > MAX_OPERANDS) {
        fprintf(stderr, "%s: %zu bytes is not 1..%ld rows of %d float64\n", path, buf.size(), MAX_OPERANDS, K);
        exit(1);
    }
    return (long)(buf.size() / row);
}

template <class F> static void run_host(const double *in, uint64_t *out, long n)
{
    if constexpr (F::HOST) {
        for (long i = 0; i < n; ++i) {
            double a[F::K];
            uint64_t o[F::M];
            for (int c = 0; c < F::K; ++c) a[c] = in[(long)c * n + i];
            F::f(a, o);
            for (int c = 0; c < F::M; ++c) out[(long)c * n + i] = o[c];
        }
    } else {
        (void)in; (void)out; (void)n;
        fprintf(stderr, "this function exists on the device only\n");
        exit(1);
    }
}
template <class F> static void run_dev(const double *in, uint64_t *out, long n, int odd)
{
    const size_t ib = (size_t)n * F::K * sizeof(double), ob = (size_t)n * F::M * sizeof(uint64_t);
    double *din = nullptr;
    uint64_t *dout = nullptr;
    CHECK_HIP(hipMalloc((void **)&din, ib));
    CHECK_HIP(hipMalloc((void **)&dout, ob));
    CHECK_HIP(hipMemcpy(din, in, ib, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(dout, out, ob, hipMemcpyHostToDevice));            // the sentinels
    hipLaunchKernelGGL(eval_kernel<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const double *)din, dout, n, odd);
    CHECK_HIP(hipGetLastError());
    CHECK_HIP(hipDeviceSynchronize());
    CHECK_HIP(hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost));
    CHECK_HIP(hipFree(din));
    CHECK_HIP(hipFree(dout));
}

// mode: 0 dev, 1 host, 2 hostdev.  Returns the number of host/device mismatches.
template <class F> static long run_function(const char *name, int mode, const char *shape, const char *in_path, const char *out_path)
{
    const std::vector<char> buf = read_file(in_path);
    const long n = operand_rows(buf, F::K, in_path);
    const double *in = (const double *)buf.data();
    int odd = 0;
    if (mode == 0) {
        if (!strcmp(shape, "full")) { if (n % 64 != 0) { fprintf(stderr, "full: %ld rows are not whole waves\n", n); exit(1); } }
        else if (!strcmp(shape, "tail")) { if (n % 64 != 37) { fprintf(stderr, "tail: %ld rows do not end in a wave of 37\n", n); exit(1); } }
        else if (!strcmp(shape, "odd")) odd = 1;
        else { fprintf(stderr, "unknown shape %s\n", shape); exit(1); }
    }
    std::vector<uint64_t> out((size_t)n * F::M, SENTINEL);
    long bad = 0;
    if (mode == 1) run_host<F>(in, out.data(), n);
    else run_dev<F>(in, out.data(), n, odd);
    if (mode == 2) {
        std::vector<uint64_t> ref((size_t)n * F::M, SENTINEL);
        run_host<F>(in, ref.data(), n);
        for (size_t k = 0; k < ref.size(); ++k) {
            const char t = F::T[k / (size_t)n];                             // NaN compares as NaN: sign and payload are free
            const bool nans = t == 'd' ? is_nan64(ref[k]) && is_nan64(out[k]) : t == 'f' ? is_nan32(ref[k]) && is_nan32(out[k]) : false;
            if (ref[k] != out[k] && !nans) {
                if (bad++ < 5) fprintf(stderr, "hostdev %s row %zu word %zu: host %016llx device %016llx\n", name, k % (size_t)n, k / (size_t)n,
                                       (unsigned long long)ref[k], (unsigned long long)out[k]);
            }
        }
        printf("hostdev %s evals=%ld mismatches=%ld\n", name, n, bad);
    } else {
        printf("%s %s rows=%ld\n", mode == 0 ? "dev" : "host", name, n);
    }
    write_file(out_path, out.data(), out.size() * sizeof(uint64_t));
    return bad;
}

static long dispatch(const char *name, int mode, const char *shape, const char *in_path, const char *out_path)
{
#define X(F, NAME) if (!strcmp(name, NAME)) return run_function<F>(name, mode, shape, in_path, out_path);
    KAT_FUNCTIONS(X)
#undef X
    fprintf(stderr, "unknown function %s\n", name);
    exit(1);
}

// rt::order_kernel on a batch of cases.  The limits are the host's (rt_plan.h: order_shape): at most 2^22 - 1 items and 2^20 - 1
// groups (the rank fields of btmp and gtmp), gshift >= wshift, nvalid <= nblocks.
static void run_order(const char *in_path, const char *out_path)
{
    const std::vector<char> buf = read_file(in_path);
    size_t pos = 0;
    auto need = [&](size_t bytes) { if (buf.size() - pos < bytes) { fprintf(stderr, "%s: truncated\n", in_path); exit(1); } };
    need(8);
    int64_t ncases;
    memcpy(&ncases, buf.data(), 8); pos = 8;
    if (ncases < 1 || ncases > 4096) { fprintf(stderr, "order: %lld cases\n", (long long)ncases); exit(1); }
    std::vector<uint32_t> all;
    for (int64_t c = 0; c < ncases; ++c) {
        need(32);
        int64_t h[4];
        memcpy(h, buf.data() + pos, 32); pos += 32;
        const int64_t nblocks = h[0], gshift = h[1], wshift = h[2], nvalid = h[3];
        if (nblocks < 1 || nblocks >= (1ll << 22) || gshift < 0 || gshift > 10 || wshift < 0 || wshift > gshift || nvalid > nblocks ||
            (nblocks >> gshift) >= (1ll << 20)) {
            fprintf(stderr, "order: case %lld out of the kernel's range\n", (long long)c);
            exit(1);
        }
        const size_t ncost = nvalid > 0 ? (size_t)nvalid : 0;
        need(ncost * 4);
        const size_t groups = (size_t)(nblocks >> gshift);
        unsigned *cost = nullptr, *gtmp = nullptr, *btmp = nullptr, *order = nullptr;
        CHECK_HIP(hipMalloc((void **)&cost, (ncost + 1) * 4));
        CHECK_HIP(hipMalloc((void **)&gtmp, (groups + 1) * 4));
        CHECK_HIP(hipMalloc((void **)&btmp, (size_t)nblocks * 4));
        CHECK_HIP(hipMalloc((void **)&order, 2 * (size_t)nblocks * 4));
        if (ncost) CHECK_HIP(hipMemcpy(cost, buf.data() + pos, ncost * 4, hipMemcpyHostToDevice));
        pos += ncost * 4;
        const size_t base = all.size();
        all.resize(base + 2 * (size_t)nblocks, SENTINEL32);
        CHECK_HIP(hipMemcpy(order, all.data() + base, 2 * (size_t)nblocks * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(rt::order_kernel, dim3(1), dim3(rt::ORDER_THREADS), 0, 0, (const unsigned *)cost, gtmp, btmp, order, (int)nblocks,
                           (int)gshift, (int)wshift, (int)nvalid);
        CHECK_HIP(hipGetLastError());
        CHECK_HIP(hipDeviceSynchronize());
        CHECK_HIP(hipMemcpy(all.data() + base, order, 2 * (size_t)nblocks * 4, hipMemcpyDeviceToHost));
        CHECK_HIP(hipFree(cost)); CHECK_HIP(hipFree(gtmp)); CHECK_HIP(hipFree(btmp)); CHECK_HIP(hipFree(order));
    }
    printf("order cases=%lld words=%zu\n", (long long)ncases, all.size());
    write_file(out_path, all.data(), all.size() * 4);
}

int main(int argc, char **argv)
{
    int i = 1;
    if (argc < 2) { fprintf(stderr, "usage: %s JOB [-- JOB ...]   (see the head of device_math_kat.hip)\n", argv[0]); return 1; }
    while (i < argc) {
        int j = i;
        while (j < argc && strcmp(argv[j], "--") != 0) ++j;
        const int na = j - i;
        const char *mode = argv[i];
        if (!strcmp(mode, "dev") && na == 5) dispatch(argv[i + 1], 0, argv[i + 2], argv[i + 3], argv[i + 4]);
        else if (!strcmp(mode, "host") && na == 4) dispatch(argv[i + 1], 1, "", argv[i + 2], argv[i + 3]);
        else if (!strcmp(mode, "hostdev") && na == 4) dispatch(argv[i + 1], 2, "", argv[i + 2], argv[i + 3]);
        else if (!strcmp(mode, "order") && na == 3) run_order(argv[i + 1], argv[i + 2]);
        else { fprintf(stderr, "bad job at argument %d\n", i); return 1; }
        fflush(stdout);
        i = j + 1;
    }
    return 0;
}
