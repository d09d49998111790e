// Host-path trace of the fused GEMV / lockstep GEMM entry points of csrc/qpal_capi.hip, without a GPU.
//
// The argument checks and launch planners of qpal_tcq_gemv, qpal_tcq_gemv_multi, qpal_lut_tc_gemv and qpal_lut_tc_gemv_multi never
// dereference a device pointer.  This program links qpal_capi.hip (compiled host-only) against stubs of everything it calls — the
// qpal::launch_* functions and the two memsets — and drives the entry points with made-up addresses.  Every stub records its name,
// its integer arguments and a 64-bit FNV-1a digest of the parameter block it was handed; a case's line is
//     <case id> <return code> <digest of the case's recorded calls>
// tests/test_capi_and_host.py compares the lines with tests/golden/capi_trace.txt: a change of the host path that computes another
// launch, zeroes another span or answers another code for any case of the sweep is caught on a machine without a GPU.
//
//     capi_trace [--reduced] [--stats] [--show id,id,...]
// --reduced: a thinned sweep (the knob runs: the QPAL_* knobs are read once per process, so each setting is a run of its own)
// --show:    also print the arguments, the recorded calls and the parameter blocks of these cases
// --stats:   calls per launcher and cases per return code, as '#' lines
//
// The digest covers the FIELDS of TcMultiParams / TcParams, not their bytes: both structs have padding, whose contents the
// language leaves open (`p = TcParams{}` need not copy it), so two host paths that compute the same launch could differ there.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <map>
#include <set>
#include <string>
#include <type_traits>
#include <vector>

#include <hip/hip_runtime.h>

#include "lut_kernels_api.h"
#include "tcq_kernels_api.h"

using namespace qpal;

namespace {

// ------------------------------------------------------------------------------------------------ digests
struct Fnv {
    uint64_t h = 0xcbf29ce484222325ull;
    void bytes(const void *p, size_t n) {
        const unsigned char *b = static_cast<const unsigned char *>(p);
        for (size_t i = 0; i < n; i++) {
            h ^= b[i];
            h *= 0x100000001b3ull;
        }
    }
    void word(uint64_t v) { bytes(&v, 8); }
};

void put(Fnv &f, const void *p) { f.word((uint64_t)(uintptr_t)p); }
void put(Fnv &f, long v) { f.word((uint64_t)v); }
void put(Fnv &f, int v) { f.word((uint64_t)(int64_t)v); }
void put(Fnv &f, float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    f.word(b);
}

void add(std::string &s, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    s += buf;
}

// (zero fields are left out of the dumps)
void show(std::string &s, const char *name, const void *p) { if (p) add(s, " %s=%#llx", name, (unsigned long long)(uintptr_t)p); }
void show(std::string &s, const char *name, long v) { if (v) add(s, " %s=%ld", name, v); }
void show(std::string &s, const char *name, int v) { if (v) add(s, " %s=%d", name, v); }
void show(std::string &s, const char *name, float v) { if (v != 0.f) add(s, " %s=%.9g", name, v); }

// every field of TcParams (tc_kernels.h), in declaration order
#define TC_FIELDS(F)                                                                                                              \
    F(out) F(wout) F(ldo) F(ldw) F(c1) F(c2) F(x) F(tab) F(n) F(k) F(nrows) F(nsc1) F(nsc2) F(st1) F(st2) F(col2) F(sk) F(nitems) \
    F(x_lds) F(cls) F(vrow0) F(kv) F(kv2) F(x_su) F(x_pre) F(x_post) F(x_rot) F(x_hadk) F(wscale) F(oscale) F(dbg) F(x_src_f32)   \
    F(x_rms_eps) F(x_rms_w) F(accumulate) F(act_su) F(act_out)
static_assert(sizeof(TcParams) == 224, "TcParams changed: list its fields in TC_FIELDS");
static_assert(sizeof(LaunchPlan) == 8 + 8 * kPlanMembers * kPlanWaves, "LaunchPlan has no padding: it is digested as bytes");

void digest(Fnv &f, const TcParams &p) {
#define F(name) put(f, p.name);
    TC_FIELDS(F)
#undef F
}

void dump(std::string &s, const TcParams &p) {
#define F(name) show(s, #name, p.name);
    TC_FIELDS(F)
#undef F
}

void digest(Fnv &f, const TcMultiParams &mp) {
    put(f, mp.njobs);
    put(f, mp.total_items);
    put(f, mp.zero_chunks);
    put(f, mp.zero);
    for (int j = 0; j < kMaxJobs; j++) put(f, mp.item_end[j]);
    put(f, mp.ncls);
    put(f, mp.items0);
    put(f, mp.cls_mask);
    for (int j = 0; j < kMaxJobs; j++) put(f, mp.row_end[j]);
    f.bytes(mp.plan, sizeof mp.plan);
    for (int j = 0; j < kMaxJobs; j++) digest(f, mp.job[j]);
}

void dump(std::string &s, const TcMultiParams &mp) {
    add(s, "    njobs=%d total_items=%d zero=%#llx zero_chunks=%d ncls=%d items0=%d cls_mask=%d\n    item_end", mp.njobs,
        mp.total_items, (unsigned long long)(uintptr_t)mp.zero, mp.zero_chunks, mp.ncls, mp.items0, mp.cls_mask);
    for (int j = 0; j < kMaxJobs; j++) add(s, " %d", mp.item_end[j]);
    add(s, "\n    row_end");
    for (int j = 0; j < kMaxJobs; j++) add(s, " %d", mp.row_end[j]);
    for (int c = 0; c < mp.ncls; c++) {
        add(s, "\n    plan[%d]: groups of %d x %d rows", c, 1 << mp.plan[c].lg_g, mp.plan[c].rg);
        for (int m = 0; m < 1 << mp.plan[c].lg_g; m++) {
            add(s, "\n      member %d:", m);
            for (int w = 0; w < kPlanWaves; w++) add(s, " %x/%x", mp.plan[c].w[m][w].a, mp.plan[c].w[m][w].b);
        }
    }
    for (int j = 0; j < mp.njobs; j++) {
        add(s, "\n    job[%d]:", j);
        dump(s, mp.job[j]);
    }
    s += "\n";
}

// ------------------------------------------------------------------------------------------------ the recorder
bool g_reduced = false;
std::string g_args;    // the current case's arguments
std::string g_trace;   // its recorded calls, one line each: what the case's digest covers
std::string g_detail;  // the same with the parameter blocks written out (--show)
bool g_show = false;
int g_calls = 0, g_fail_at = -1;  // the g_fail_at-th recorded call of the case reports an error
std::map<std::string, int> g_launches, g_codes;

template <class P>
int note(const char *name, const P &p, std::initializer_list<int> ints, hipStream_t stream) {
    Fnv f;
    digest(f, p);
    std::string line = name;
    line += "(";
    for (int v : ints) add(line, "%d,", v);
    add(line, "stream=%#llx) params=%016llx\n", (unsigned long long)(uintptr_t)stream, (unsigned long long)f.h);
    g_trace += line;
    if (g_show) {
        g_detail += "  " + line;
        dump(g_detail, p);
        if constexpr (std::is_same<P, TcParams>::value) g_detail += "\n";
    }
    g_launches[name]++;
    return g_calls++ == g_fail_at ? (int)hipErrorLaunchFailure : 0;
}

hipError_t note_memset(const char *name, const std::string &what) {
    const std::string line = std::string(name) + "(" + what + ")\n";
    g_trace += line;
    if (g_show) g_detail += "  " + line;
    g_launches[name]++;
    return g_calls++ == g_fail_at ? hipErrorInvalidValue : hipSuccess;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ stubs of what qpal_capi.hip calls
namespace qpal {
int launch_tcq_gemv(const TcMultiParams &p, int S, int KV1, int KV2, int nbg, int grid, hipStream_t s) {
    return note("launch_tcq_gemv", p, {S, KV1, KV2, nbg, grid}, s);
}
#define TCQ_GEMM_STUB(NBG)                                                                                       \
    int launch_tcq_gemm_nbg##NBG(const TcMultiParams &p, int S, int KV1, int KV2, int grid, hipStream_t s) {     \
        return note("launch_tcq_gemm_nbg" #NBG, p, {S, KV1, KV2, grid}, s);                                      \
    }
TCQ_GEMM_STUB(1)
TCQ_GEMM_STUB(2)
TCQ_GEMM_STUB(4)
TCQ_GEMM_STUB(8)
TCQ_GEMM_STUB(10)
TCQ_GEMM_STUB(16)
int launch_tcq_gemv_any(const TcMultiParams &p, int S, int grid, hipStream_t s) { return note("launch_tcq_gemv_any", p, {S, grid}, s); }
int launch_tcq_dequant(const TcParams &p, int S, int KV1, int KV2, int grid, hipStream_t s) {
    return note("launch_tcq_dequant", p, {S, KV1, KV2, grid}, s);
}
int launch_lut_tc_gemv(const TcMultiParams &p, int bits, int vec, int nbg, int grid, hipStream_t s) {
    return note("launch_lut_tc_gemv", p, {bits, vec, nbg, grid}, s);
}
int launch_lut_tc_gemm(const TcMultiParams &p, int bits, int vec, int nbg, int grid, hipStream_t s) {
    return note("launch_lut_tc_gemm", p, {bits, vec, nbg, grid}, s);
}
int launch_lut_tc_dequant(const TcParams &p, int bits, int vec, int grid, hipStream_t s) {
    return note("launch_lut_tc_dequant", p, {bits, vec, grid}, s);
}
// (the SIMT entries are not part of the sweep: their stubs only satisfy the linker)
int launch_simt_gemv(const SimtParams &, int, int, int, const SimtGeometry &, hipStream_t) { return 0; }
int launch_simt_dequant(const SimtParams &, int, int, int, hipStream_t) { return 0; }
int launch_tc_to_simt(uint32_t *, const uint32_t *, int, int, int, int, hipStream_t) { return 0; }
}  // namespace qpal

extern "C" {
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t stream) {
    std::string w;
    add(w, "%#llx,%d,%zu,stream=%#llx", (unsigned long long)(uintptr_t)dst, value, bytes, (unsigned long long)(uintptr_t)stream);
    return note_memset("hipMemsetAsync", w);
}
hipError_t hipMemset2DAsync(void *dst, size_t pitch, int value, size_t width, size_t height, hipStream_t stream) {
    std::string w;
    add(w, "%#llx,pitch=%zu,%d,%zu x %zu,stream=%#llx", (unsigned long long)(uintptr_t)dst, pitch, value, width, height,
        (unsigned long long)(uintptr_t)stream);
    return note_memset("hipMemset2DAsync", w);
}
const char *hipGetErrorString(hipError_t) { return "hip error (stub)"; }
}

namespace {

// ------------------------------------------------------------------------------------------------ cases
std::set<std::string> g_show_ids;
std::string g_id;

void begin(const char *prefix, int number) {
    char id[32];
    snprintf(id, sizeof id, "%s%04d", prefix, number);
    g_id = id;
    g_args.clear();
    g_trace.clear();
    g_detail.clear();
    g_calls = 0;
    g_fail_at = -1;
    g_show = g_show_ids.count(g_id) != 0;
}

void end(int rc) {
    Fnv f;
    f.bytes(g_trace.data(), g_trace.size());
    printf("%s %d %016llx\n", g_id.c_str(), rc, (unsigned long long)f.h);
    char code[16];
    snprintf(code, sizeof code, "%d", rc);
    g_codes[code]++;
    if (g_show) printf("  args: %s\n%s", g_args.c_str(), g_detail.c_str());
}

// a fixed generator: the sweep is the same on every machine
uint32_t g_seed = 20261019u;
uint32_t rnd() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return g_seed >> 8;
}
int pick(int n) { return (int)(rnd() % (uint32_t)n); }
bool chance(int percent) { return pick(100) < percent; }
template <class T, size_t N>
T one_of(const T (&v)[N]) { return v[pick((int)N)]; }

// made-up addresses, never dereferenced
char *at(uintptr_t a) { return reinterpret_cast<char *>(a); }
char *const OUT = at(0x10000000), *const W1 = at(0x20000000), *const W2 = at(0x30000000), *const X16 = at(0x40000000),
            *const X32 = at(0x50000000), *const TAB = at(0x60000000), *const WSC = at(0x61000000), *const SU = at(0x62000000),
            *const RMSW = at(0x62100000), *const HADK = at(0x62200000), *const ACT = at(0x63000000), *const ACTSU = at(0x64000000),
            *const PREZERO = at(0x65000000), *const STREAM = at(0x5000);
constexpr size_t kJobStride = 0x1000000;  // (the largest output of the sweep, [128][28672] fp32, is 14 MiB)
char *x_of(int k, bool f32 = false) { return (f32 ? X32 : X16) + (size_t)(k / 32 % 61) * 0x400000; }

const int kNs[] = {1, 2, 3, 4, 7, 8, 9, 16, 17, 32, 33, 64, 65, 80, 81, 128};
const int kNsFew[] = {1, 2, 9, 65, 128};
const int kMK[][2] = {{32, 32}, {64, 64}, {96, 160}, {1024, 4096}, {4096, 4096}, {6144, 4096}, {4096, 14336}, {28672, 4096}, {8192, 8192}};
// The GEMV planner enumerates every (group, rows) candidate of a launch: 2 ... 70 ms of host time per call at these k, against
// microseconds for the lockstep planner and the argument checks.  Batches below the lockstep kernel's threshold (n < 4) are
// therefore swept on fewer, smaller shapes, and so is the whole reduced sweep (QPAL_GEMM_MIN_BATCH = 128 sends it all there).
bool plans_gemv(int n) { return n < 4 || g_reduced; }
int std_k(int n) { return plans_gemv(n) ? 512 : 4096; }
const int kSKV[][2] = {{9, 2}, {9, 6}, {9, 8}, {9, 10}, {10, 8}, {10, 10}, {11, 9}};
const int kLut[][2] = {{2, 1}, {4, 1}, {6, 1}, {7, 1}, {8, 1}, {3, 2}, {8, 2}, {12, 2}};

template <class T, size_t N>
bool among(T v, const T (&set)[N]) {
    for (T s : set)
        if (s == v) return true;
    return false;
}

// ---- the single-layer entry points
int tcq_one(int m, int n, int k, int S, int KV, int split, const void *x) {
    add(g_args, "qpal_tcq_gemv m=%d n=%d k=%d S=%d KV1=%d split=%d x=%#llx", m, n, k, S, KV, split, (unsigned long long)(uintptr_t)x);
    return qpal_tcq_gemv(reinterpret_cast<float *>(OUT), W1, split ? W2 : nullptr, x, TAB, m, n, k, S, KV, split ? KV + 1 : 0, split, STREAM);
}

void sweep_tcq_single() {
    int id = 0;
    for (size_t c = 0; c < 7; c++) {
        const bool dense = c == 1 || (c == 4 && !g_reduced);  // every batch for (9, 6) and (10, 8); three batches for the other codecs
        if (g_reduced && !dense && c != 6) continue;
        for (int split = 0; split < 3; split++)
            for (int n : kNs) {
                const int few[] = {1, 9, 128};
                if (!dense && !among(n, few)) continue;
                if (g_reduced && !among(n, kNsFew)) continue;
                const bool all_shapes = !plans_gemv(n) || (c == 1 && n == 1 && !g_reduced) || (c == 4 && n > 1 && split == 0 && !g_reduced);
                for (const auto &mk : kMK) {
                    if (!all_shapes && !among(mk[0], {64, 96}) && !(mk[0] == 1024 && (c == 1 || (c == 4 && n == 1)))) continue;
                    if (plans_gemv(n) && split == QPAL_SPLIT_ROWS && mk[1] >= 8192) continue;  // (two plans of the widest rows)
                    begin("tg", id++);
                    end(tcq_one(mk[0], n, mk[1], kSKV[c][0], kSKV[c][1], split, X16));
                }
            }
    }
    // what the lockstep kernel declines: x aligned to 8 but not to 16 bytes; k % 8 != 0 (no such k passes k % 32 == 0)
    for (int n : kNs)
        for (int split = 0; split < 3; split++)
            for (const auto &mk : {kMK[1], kMK[3], kMK[6]}) {
                const int heavy[] = {4, 33, 65, 128};  // (n <= 64 plans a GEMV launch here)
                if (mk[0] != 64 && (g_reduced || !among(n, heavy) || (mk[1] == 14336 && split != 2))) continue;
                if (g_reduced && !among(n, kNsFew)) continue;
                begin("ta", id++);
                end(tcq_one(mk[0], n, mk[1], 9, 6, split, X16 + 8));
            }
    for (int k : {36, 4100, 4104}) {
        begin("ta", id++);
        end(tcq_one(1024, 16, k, 9, 6, 0, X16));
    }
    // a memset or a launch that fails ends the call with its code (row halves: the second launch is not started)
    for (int n : {1, 64})
        for (int split = 0; split < 3; split++)
            for (int fail = 0; fail < 4; fail++) {
                begin("tf", id++);
                g_fail_at = fail;
                add(g_args, "call %d fails: ", fail);
                end(tcq_one(1024, n, n == 1 ? 512 : 4096, 9, 6, split, X16));
            }
    // argument errors of the single entry
    struct Bad { const char *what; int m, n, k, S, KV, split; const void *out, *c1, *c2, *x, *tab; };
    const Bad bad[] = {
        {"out null", 1024, 1, 4096, 9, 6, 0, nullptr, W1, nullptr, X16, TAB},
        {"c1 null", 1024, 1, 4096, 9, 6, 0, OUT, nullptr, nullptr, X16, TAB},
        {"c2 null, split", 1024, 1, 4096, 9, 6, 2, OUT, W1, nullptr, X16, TAB},
        {"x null", 1024, 1, 4096, 9, 6, 0, OUT, W1, nullptr, nullptr, TAB},
        {"tlut null", 1024, 1, 4096, 9, 6, 0, OUT, W1, nullptr, X16, nullptr},
        {"m % 32", 1000, 1, 4096, 9, 6, 0, OUT, W1, nullptr, X16, TAB},
        {"m % 32, out null", 1000, 1, 4096, 9, 6, 0, nullptr, W1, nullptr, X16, TAB},
        {"n = 0", 1024, 0, 4096, 9, 6, 0, OUT, W1, nullptr, X16, TAB},
        {"n = 129", 1024, 129, 4096, 9, 6, 0, OUT, W1, nullptr, X16, TAB},
        {"n = 129, x misaligned", 1024, 129, 4096, 9, 6, 0, OUT, W1, nullptr, X16 + 4, TAB},
        {"x misaligned", 1024, 1, 4096, 9, 6, 0, OUT, W1, nullptr, X16 + 4, TAB},
        {"out misaligned", 1024, 1, 4096, 9, 6, 0, OUT + 2, W1, nullptr, X16, TAB},
        {"c1 misaligned", 1024, 1, 4096, 9, 6, 0, OUT, W1 + 2, nullptr, X16, TAB},
        {"c1 misaligned, KV", 1024, 1, 4096, 9, 11, 0, OUT, W1 + 2, nullptr, X16, TAB},
        {"split 3", 1024, 1, 4096, 9, 6, 3, OUT, W1, W2, X16, TAB},
        {"S 12", 1024, 1, 4096, 12, 6, 0, OUT, W1, nullptr, X16, TAB},
        {"KV 11", 1024, 1, 4096, 9, 11, 0, OUT, W1, nullptr, X16, TAB},
        {"KV 7 at S 10", 1024, 1, 4096, 10, 7, 0, OUT, W1, nullptr, X16, TAB},
    };
    for (const Bad &b : bad) {
        begin("tb", id++);
        add(g_args, "qpal_tcq_gemv %s", b.what);
        end(qpal_tcq_gemv((float *)b.out, b.c1, b.c2, b.x, b.tab, b.m, b.n, b.k, b.S, b.KV, b.split ? b.KV + 1 : 0, b.split, STREAM));
    }
}

void sweep_lut_single() {
    int id = 0;
    for (size_t c = 0; c < 8; c++) {
        const bool dense = c == 1 || (c == 7 && !g_reduced);  // every batch for (4, 1) and for (12, 2) with its 128 KiB image
        if (g_reduced && !dense && c != 2) continue;
        for (int n : kNs) {
            const int few[] = {1, 9, 64, 65, 80, 128};
            if (!dense && !among(n, few)) continue;
            if (!dense && n == 1 && c != 2 && c != 5) continue;
            if (g_reduced && !among(n, kNsFew)) continue;
            const bool all_shapes = !plans_gemv(n) || (c == 1 && n == 1 && !g_reduced);
            for (const auto &mk : kMK) {
                if (!all_shapes && !among(mk[0], {64, 96}) && !(mk[0] == 1024 && (c == 1 || (c == 7 && n == 1)))) continue;
                begin("lg", id++);
                add(g_args, "qpal_lut_tc_gemv m=%d n=%d k=%d bits=%d vec=%d", mk[0], n, mk[1], kLut[c][0], kLut[c][1]);
                end(qpal_lut_tc_gemv((float *)OUT, W1, X16, TAB, mk[0], n, mk[1], kLut[c][0], kLut[c][1], STREAM));
            }
        }
    }
    for (int n : kNs)
        for (const auto &bv : {kLut[1], kLut[7]}) {
            begin("la", id++);
            const int heavy[] = {4, 33, 65, 128};
            const int k = among(n, heavy) && !g_reduced ? 4096 : 256;
            add(g_args, "qpal_lut_tc_gemv m=1024 n=%d k=%d bits=%d vec=%d x + 8", n, k, bv[0], bv[1]);
            end(qpal_lut_tc_gemv((float *)OUT, W1, X16 + 8, TAB, 1024, n, k, bv[0], bv[1], STREAM));
        }
    for (int fail = 0; fail < 3; fail++) {
        begin("lf", id++);
        g_fail_at = fail;
        add(g_args, "call %d fails: qpal_lut_tc_gemv m=1024 n=64 k=4096 bits=4 vec=1", fail);
        end(qpal_lut_tc_gemv((float *)OUT, W1, X16, TAB, 1024, 64, 4096, 4, 1, STREAM));
    }
    struct Bad { const char *what; int m, n, k, bits, vec; const void *out, *q, *x, *lut; };
    const Bad bad[] = {
        {"out null", 1024, 1, 4096, 4, 1, nullptr, W1, X16, TAB},   {"qweight null", 1024, 1, 4096, 4, 1, OUT, nullptr, X16, TAB},
        {"x null", 1024, 1, 4096, 4, 1, OUT, W1, nullptr, TAB},     {"lut null", 1024, 1, 4096, 4, 1, OUT, W1, X16, nullptr},
        {"m % 32", 1000, 1, 4096, 4, 1, OUT, W1, X16, TAB},         {"k % 32", 1024, 1, 4100, 4, 1, OUT, W1, X16, TAB},
        {"n = 0", 1024, 0, 4096, 4, 1, OUT, W1, X16, TAB},          {"n = 129", 1024, 129, 4096, 4, 1, OUT, W1, X16, TAB},
        {"bits 9, vec 1", 1024, 1, 4096, 9, 1, OUT, W1, X16, TAB},  {"bits 13, vec 2", 1024, 1, 4096, 13, 2, OUT, W1, X16, TAB},
        {"vec 4", 1024, 1, 4096, 8, 4, OUT, W1, X16, TAB},          {"bits * k % 64", 1024, 1, 32, 3, 2, OUT, W1, X16, TAB},
        {"x misaligned", 1024, 1, 4096, 4, 1, OUT, W1, X16 + 4, TAB}, {"out misaligned", 1024, 1, 4096, 4, 1, OUT + 2, W1, X16, TAB},
        {"qweight misaligned", 1024, 1, 4096, 4, 1, OUT, W1 + 2, X16, TAB}, {"lut misaligned, bits 9", 1024, 1, 4096, 9, 1, OUT, W1, X16, TAB + 2},
        {"m % 32, x null", 1000, 1, 4096, 4, 1, OUT, W1, nullptr, TAB},
    };
    for (const Bad &b : bad) {
        begin("lb", id++);
        add(g_args, "qpal_lut_tc_gemv %s", b.what);
        end(qpal_lut_tc_gemv((float *)b.out, b.q, b.x, b.lut, b.m, b.n, b.k, b.bits, b.vec, STREAM));
    }
}

// ---- the multi-job entry points: one launch description for both families
template <class J>
struct Launch {
    static constexpr bool kTcq = std::is_same<J, qpal_tcq_job>::value;
    J j[kMaxJobs + 1] = {};
    int nj = 0, n = 1;
    int S = 9, KV1 = 6, KV2 = 0, split = 0;  // TCQ
    int bits = 4, vec = 1;                   // LUT
    void *pz = nullptr;
    long pzb = 0;
    bool no_jobs = false;
};
using TcqLaunch = Launch<qpal_tcq_job>;
using LutLaunch = Launch<qpal_lut_job>;

enum Layout { kContig, kApart, kWide };  // outputs that follow each other in memory, that do not, column blocks of one wider buffer

template <class J>
void add_job(Launch<J> &t, int m, int k) {
    J &jb = t.j[t.nj];
    jb = J{};
    const size_t o = (size_t)t.nj * kJobStride;
    jb.out = reinterpret_cast<float *>(OUT + o);
    if constexpr (Launch<J>::kTcq) {
        jb.c1 = W1 + o;
        jb.c2 = t.split == QPAL_SPLIT_COLS ? W2 + o : nullptr;
        jb.tlut = TAB;
    } else {
        jb.qweight = W1 + o;
        jb.lut = TAB;
    }
    jb.x = x_of(k);
    jb.m = m;
    jb.k = k;
    jb.oscale = 1.0f;
    jb.x_post = 1.0f;
    t.nj++;
}

template <class J>
void lay_out(Launch<J> &t, Layout lay) {
    long total = 0;
    for (int j = 0; j < t.nj; j++) total += t.j[j].m;
    size_t off = 0;
    for (int j = 0; j < t.nj; j++) {
        J &jb = t.j[j];
        if (lay == kApart) continue;  // (add_job's)
        jb.out = reinterpret_cast<float *>(OUT + off);
        if (lay == kContig) off += sizeof(float) * (size_t)t.n * jb.m;
        else {
            off += sizeof(float) * (size_t)jb.m;
            jb.ldo = total;
        }
    }
}

// the rotation (x_had) on job j: sign vector, fp32 input, RMSNorm
template <class J>
void rotate(J &jb, bool su, bool f32, bool eps, bool rms_w) {
    jb.x_had = 1;
    jb.x_post = 0.5f;
    jb.x_su = su ? SU : nullptr;
    if (f32) {
        jb.x_f32 = x_of(jb.k, true);
        jb.x = nullptr;
    }
    jb.x_rms_eps = eps ? 1e-5f : 0.f;
    jb.x_rms_w = rms_w ? RMSW : nullptr;
}
template <class J>
void rotate28(J &jb, bool su) {
    jb.x_had = 1;
    jb.x_post = 0.5f;
    jb.x_su = su ? SU : nullptr;
    jb.x_hadk = HADK;
    jb.x_K = 28;
}
template <class J>
void swiglu(J &jb, int j, bool su, bool keep_out) {
    jb.act_out = ACT + (size_t)j * 0x10000;
    jb.act_su = su ? ACTSU + (size_t)j * 0x10000 : nullptr;
    if (!keep_out) jb.out = nullptr;
}

template <class J>
void describe(const Launch<J> &t) {
    if constexpr (Launch<J>::kTcq) add(g_args, "qpal_tcq_gemv_multi njobs=%d n=%d S=%d KV1=%d KV2=%d split=%d", t.nj, t.n, t.S, t.KV1, t.KV2, t.split);
    else add(g_args, "qpal_lut_tc_gemv_multi njobs=%d n=%d bits=%d vec=%d", t.nj, t.n, t.bits, t.vec);
    add(g_args, " prezero=%#llx/%ld%s", (unsigned long long)(uintptr_t)t.pz, t.pzb, t.no_jobs ? " jobs=NULL" : "");
    for (int j = 0; j < t.nj && j <= kMaxJobs; j++) {
        const J &jb = t.j[j];
        add(g_args, "\n    job %d:", j);
#define A(name) show(g_args, #name, jb.name);
        if constexpr (Launch<J>::kTcq) { A(out) A(c1) A(c2) A(x) A(tlut) A(kv) A(kv2) }
        else { A(out) A(qweight) A(x) A(lut) }
        A(m) A(k) A(out_zeroed) A(wscale) A(oscale) A(ldo) A(x_had) A(x_post) A(x_su) A(x_f32) A(x_rms_eps) A(x_rms_w) A(accumulate)
        A(act_out) A(x_hadk) A(x_K) A(act_su)
#undef A
    }
}

template <class J>
int call(const Launch<J> &t) {
    describe(t);
    if constexpr (Launch<J>::kTcq)
        return qpal_tcq_gemv_multi(t.no_jobs ? nullptr : t.j, t.nj, t.n, t.S, t.KV1, t.KV2, t.split, t.pz, t.pzb, STREAM);
    else
        return qpal_lut_tc_gemv_multi(t.no_jobs ? nullptr : t.j, t.nj, t.n, t.bits, t.vec, t.pz, t.pzb, STREAM);
}

template <class J>
Launch<J> launch_of(int nj, int n, int m, int k, int split = 0) {
    Launch<J> t;
    t.n = n;
    t.split = split;
    t.KV2 = split ? t.KV1 + 1 : 0;
    for (int j = 0; j < nj; j++) add_job(t, m, k);
    return t;
}

// the job variations both families share
template <class J>
void sweep_multi_shared(const char *prefix) {
    int id = 0;
    auto run = [&](const Launch<J> &t) {
        begin(prefix, id++);
        end(call(t));
    };
    const int ns[] = {1, 2, 4, 8, 9, 16, 33, 64, 81, 128}, ns_few[] = {1, 4, 16, 64};
    // 1 to 8 jobs of one k; the three output layouts; out_zeroed 0 and 1
    for (int nj = 1; nj <= kMaxJobs; nj++)
        for (int n : ns) {
            if (g_reduced && !among(n, ns_few)) continue;
            for (int lay = 0; lay < 3; lay++)
                for (int z = 0; z < 2; z++) {
                    if ((nj == 5 || nj == 7) && !among(n, ns_few)) continue;
                    if (plans_gemv(n) && (nj == 4 || nj == 6)) continue;
                    if (g_reduced && ((lay + z) % 2 || (nj > 2 && nj < 8))) continue;
                    Launch<J> t = launch_of<J>(nj, n, nj % 3 == 0 ? 4096 : 1024, nj == 2 && lay == 0 && !g_reduced ? 4096 : std_k(n));
                    if (nj > 1) t.j[1].m = 6144;
                    lay_out(t, (Layout)lay);
                    for (int j = 0; j < nj; j++) t.j[j].out_zeroed = z;
                    run(t);
                }
        }
    // the 128 KiB images (LUT) / the other codebook sizes (TCQ) at every batch group
    for (int n : kNs)
        for (int v = 0; v < 3; v++) {
            if (g_reduced && !among(n, kNsFew)) continue;
            Launch<J> t = launch_of<J>(2, n, 1024, std_k(n));
            if constexpr (Launch<J>::kTcq) { t.S = 9 + v; t.KV1 = v == 0 ? 2 : 9; }
            else { t.bits = v == 0 ? 12 : v == 1 ? 6 : 8; t.vec = v == 0 ? 2 : 1; }
            lay_out(t, kContig);
            run(t);
        }
    // one, two and more than two distinct k (a launch per geometry; prezero goes to the first one), accumulate, wscale, oscale
    const std::vector<std::vector<int>> kss = {{4096, 14336}, {4096, 4096, 14336}, {4096, 14336, 4096, 14336}, {2048, 4096, 8192},
                                               {64, 4096, 8192, 14336, 64, 4096}, {8192, 64, 4096, 64, 8192, 14336, 2048, 32}};
    for (const auto &ks : kss)
        for (int n : ns_few)
            for (int v = 0; v < 4; v++) {
                const bool real = v == 3 && ks.size() == 3 && !g_reduced;  // (a GEMV launch of real widths: one per list of three)
                if (plans_gemv(n) && ks.size() > 3 && v != 3) continue;
                Launch<J> t = launch_of<J>(0, n, 0, 0);
                for (size_t j = 0; j < ks.size(); j++) add_job(t, j % 2 ? 1024 : 4096, plans_gemv(n) && !real ? ks[j] / 16 : ks[j]);
                lay_out(t, v == 3 ? kWide : v == 2 ? kApart : kContig);
                if (v >= 1) { t.pz = PREZERO; t.pzb = 4096; }
                if (v >= 2)
                    for (int j = 0; j < t.nj; j++) {
                        t.j[j].accumulate = j % 2;
                        t.j[j].out_zeroed = j == 2;
                        t.j[j].wscale = WSC + j * 0x10000;
                        t.j[j].oscale = j % 3 ? 0.25f : 0.f;
                    }
                run(t);
            }
    // accumulate, on every batch group
    for (int n : ns)
        for (int v = 0; v < 3; v++) {
            if (g_reduced && !among(n, ns_few)) continue;
            Launch<J> t = launch_of<J>(2, n, v == 2 ? 4096 : 1024, g_reduced ? 512 : v == 2 && n != 2 ? 14336 : std_k(n));
            lay_out(t, kContig);
            t.j[0].accumulate = 1;
            t.j[1].accumulate = v == 0;
            t.j[1].out_zeroed = v == 1;
            run(t);
        }
    // prezero sizes
    for (long bytes : {16L, 4096L, 1L << 20})
        for (int n : {1, 64}) {
            Launch<J> t = launch_of<J>(2, n, 1024, std_k(n));
            t.pz = PREZERO;
            t.pzb = bytes;
            run(t);
        }
    // the fused rotation: k 2048 and 4096, with and without sign vector, fp32 input, RMSNorm and its weight; batch 1 only
    for (int k : {2048, 4096, 8192})
        for (int nj : {1, 3})
            for (int bits = 0; bits < 16; bits++) {
                if (k == 8192 && bits % 5) continue;
                const int eight[] = {0, 1, 2, 4, 6, 8, 9, 15};
                if ((nj == 3 && bits % 5) || (k == 2048 && bits % 3) || !among(bits, eight)) continue;
                if (g_reduced && (nj == 3 || k == 2048 || bits % 15)) continue;
                Launch<J> t = launch_of<J>(nj, 1, 1024, k);
                lay_out(t, kContig);
                for (int j = 0; j < nj; j++) rotate(t.j[j], bits & 1, bits & 2, bits & 4, bits & 8);
                run(t);
            }
    for (int n : {2, 8, 9, 32, 64, 128})
        for (int f32 = 0; f32 < 2; f32++) {
            Launch<J> t = launch_of<J>(2, n, 1024, 4096);
            for (int j = 0; j < 2; j++) rotate(t.j[j], true, f32, false, false);
            run(t);
        }
    // the SwiGLU epilogue (m % 64 == 0), with and without its sign vector, out kept or null; beside a plain job; two of them
    for (int m : {64, 128, 1024, 28672})
        for (int v = 0; v < 8; v++) {
            if (g_reduced && (m == 128 || v % 3)) continue;
            Launch<J> t = launch_of<J>(1 + (v >> 2), 1, m, 4096);
            for (int j = 0; j < t.nj; j++) rotate(t.j[j], true, true, true, true);
            swiglu(t.j[0], 0, v & 1, v & 2);
            if (t.nj > 1 && (v & 1)) swiglu(t.j[1], 1, true, false);
            for (int j = 0; j < t.nj; j++) t.j[j].out_zeroed = v & 1;
            run(t);
        }
    // the 14336-wide rotation (K = 28)
    for (int nj : {1, 2})
        for (int v = 0; v < 4; v++) {
            if ((nj == 2 && v != 3) || v == 2 || (g_reduced && v != 3)) continue;
            Launch<J> t = launch_of<J>(nj, 1, 4096, 14336);
            if constexpr (!Launch<J>::kTcq) { t.bits = v & 2 ? 12 : 8; t.vec = 2; }  // (the 32 KiB image of (8, 2) cannot lend the rotation 40 KiB)
            else t.j[0].out_zeroed = v >> 1;
            lay_out(t, kContig);
            for (int j = 0; j < nj; j++) rotate28(t.j[j], v & 1);
            run(t);
        }
    // a memset or a launch that fails
    for (int n : {1, 64})
        for (int fail = 0; fail < 3; fail++) {
            Launch<J> t = launch_of<J>(3, n, 1024, std_k(n));
            t.j[2].k = 2 * std_k(n);
            t.j[2].x = x_of(t.j[2].k);
            t.j[1].out = reinterpret_cast<float *>(OUT + 2 * kJobStride + 64);  // three spans
            begin(prefix, id++);
            g_fail_at = fail;
            add(g_args, "call %d fails: ", fail);
            end(call(t));
        }
}

// what only the TCQ entry has: split COLS, per-job KV (the any-KV kernel), kv2 with c2
void sweep_tcq_multi_own() {
    int id = 0;
    auto run = [&](const TcqLaunch &t) {
        begin("mk", id++);
        end(call(t));
    };
    for (const auto &skv : kSKV)
        for (int nj : {1, 2, 3})
            for (int n : {1, 8, 9, 64, 128}) {
                if (g_reduced && (nj == 2 || n == 8)) continue;
                if (plans_gemv(n) && skv[1] != 6 && nj != 2) continue;
                const bool real = skv[1] == 6 && !g_reduced;  // (two o_proj / down_proj sized jobs at batch 1: rows shared, one memset)
                TcqLaunch t = launch_of<qpal_tcq_job>(0, n, 0, 0, QPAL_SPLIT_COLS);
                t.S = skv[0];
                t.KV1 = skv[1];
                t.KV2 = skv[1] + 1;
                for (int j = 0; j < nj; j++) add_job(t, j ? 1024 : 4096, (j == 2 ? 14336 : 4096) / (plans_gemv(n) && !real ? 8 : 1));
                lay_out(t, kContig);
                run(t);
            }
    // jobs with their own KV; a column-split job (kv2, c2) beside single-stream ones; three geometries with them
    const int kvs[][4] = {{4, 6, 8, 0}, {6, 6, 6, 6}, {0, 0, 5, 0}, {2, 8, 3, 7}};
    for (const auto &kv : kvs)
        for (int n : {1, 4, 8})
            for (int v = 0; v < 4; v++) {
                TcqLaunch t = launch_of<qpal_tcq_job>(0, n, 0, 0);
                if (g_reduced && n == 4) continue;
                for (int j = 0; j < 4; j++) {
                    add_job(t, j ? 1024 : 4096, (v == 3 && j == 3 ? 14336 : 4096) / (n == 8 && kv[0] == 4 && !g_reduced ? 1 : 8));
                    t.j[j].kv = kv[j];
                }
                if (v >= 1) { t.j[0].kv = 6; t.j[0].kv2 = 7; t.j[0].c2 = W2; }
                if (v >= 2) { t.j[2].kv = 3; t.j[2].kv2 = 4; t.j[2].c2 = W2 + kJobStride; t.j[2].out_zeroed = 1; }
                lay_out(t, v % 2 ? kContig : kApart);
                run(t);
            }
    for (int S : {10, 11})
        for (int v = 0; v < 3; v++) {
            TcqLaunch t = launch_of<qpal_tcq_job>(2, 1, 1024, 512);
            t.S = S;
            t.KV1 = 9;
            t.j[1].kv = v == 0 ? 10 : v == 1 ? 8 : 9;
            if (v == 2) { t.j[1].kv2 = 10; t.j[1].c2 = W2; }
            run(t);
        }
}

// ---- invalid calls: every rule on its own, and every pair of rules (which code wins is part of the contract)
template <class J>
void sweep_invalid(const char *prefix) {
    using L = Launch<J>;
    struct Rule { const char *what; void (*apply)(L &); };
    std::vector<Rule> rules = {
        {"jobs null", [](L &t) { t.no_jobs = true; }},
        {"njobs 0", [](L &t) { t.nj = 0; }},
        {"njobs 9", [](L &t) { while (t.nj < 9) { t.j[t.nj] = t.j[0]; t.nj++; } }},
        {"n 0", [](L &t) { t.n = 0; }},
        {"n 129", [](L &t) { t.n = 129; }},
        {"prezero misaligned", [](L &t) { t.pz = PREZERO + 8; t.pzb = 64; }},
        {"prezero bytes % 16", [](L &t) { t.pz = PREZERO; t.pzb = 24; }},
        {"prezero null", [](L &t) { t.pz = nullptr; t.pzb = 64; }},
        {"out null", [](L &t) { t.j[1].out = nullptr; }},
        {"x null", [](L &t) { t.j[0].x = nullptr; }},
        {"m % 32", [](L &t) { t.j[1].m = 1000; }},
        {"k % 32", [](L &t) { t.j[0].k = 4100; t.j[1].k = 4100; }},
        {"ldo < m", [](L &t) { t.j[1].ldo = 512; }},
        {"x misaligned", [](L &t) { t.j[0].x = X16 + 4; t.j[1].x = X16 + 4; }},
        {"out misaligned", [](L &t) { t.j[0].out = reinterpret_cast<float *>(OUT + 2); }},
        {"wscale misaligned", [](L &t) { t.j[1].wscale = WSC + 1; }},
        {"x_su misaligned", [](L &t) { for (int j = 0; j < 2; j++) { rotate(t.j[j], true, false, false, false); t.j[j].x_su = SU + 8; } }},
        {"x_rms_w misaligned", [](L &t) { for (int j = 0; j < 2; j++) { rotate(t.j[j], true, false, true, true); t.j[j].x_rms_w = RMSW + 8; } }},
        {"x_f32 without x_had", [](L &t) { t.j[0].x_f32 = x_of(4096, true); }},
        {"x_rms_eps without x_had", [](L &t) { t.j[1].x_rms_eps = 1e-5f; }},
        {"x_had at n 2", [](L &t) { t.n = 2; for (int j = 0; j < 2; j++) rotate(t.j[j], true, false, false, false); }},
        {"x_had at n 32", [](L &t) { t.n = 32; for (int j = 0; j < 2; j++) rotate(t.j[j], false, false, false, false); }},
        {"x_had at k 8192", [](L &t) { for (int j = 0; j < 2; j++) { t.j[j].k = 8192; rotate(t.j[j], true, false, false, false); } }},
        {"x_had, x 8-aligned", [](L &t) { for (int j = 0; j < 2; j++) { rotate(t.j[j], true, false, false, false); t.j[j].x = X16 + 8; } }},
        {"act_out at n 2", [](L &t) { t.n = 2; for (int j = 0; j < 2; j++) rotate(t.j[j], true, false, false, false); swiglu(t.j[0], 0, true, false); }},
        {"act_out with accumulate", [](L &t) { for (int j = 0; j < 2; j++) rotate(t.j[j], true, false, false, false); swiglu(t.j[0], 0, true, true); t.j[0].accumulate = 1; }},
        {"act_out with m % 64", [](L &t) { for (int j = 0; j < 2; j++) rotate(t.j[j], true, false, false, false); t.j[1].m = 96; swiglu(t.j[1], 1, false, false); }},
        {"act_out without x_had", [](L &t) { swiglu(t.j[1], 1, true, false); }},
        {"act_out misaligned", [](L &t) { for (int j = 0; j < 2; j++) rotate(t.j[j], true, false, false, false); swiglu(t.j[0], 0, true, false); t.j[0].act_out = ACT + 1; }},
        {"shared x: x_su", [](L &t) { for (int j = 0; j < 2; j++) rotate(t.j[j], true, false, false, false); t.j[1].x_su = SU + 0x10000; }},
        {"shared x: x_post", [](L &t) { for (int j = 0; j < 2; j++) rotate(t.j[j], true, false, false, false); t.j[1].x_post = 0.25f; }},
        {"shared x: x_had", [](L &t) { rotate(t.j[1], true, false, false, false); }},
        {"shared x: x_rms_eps", [](L &t) { for (int j = 0; j < 2; j++) rotate(t.j[j], true, true, true, true); t.j[1].x_rms_eps = 1e-6f; }},
        {"shared x: x_rms_w", [](L &t) { for (int j = 0; j < 2; j++) rotate(t.j[j], true, true, true, true); t.j[1].x_rms_w = RMSW + 0x10000; }},
        {"shared x: k", [](L &t) { t.j[1].k = 2048; }},
        {"shared x: x_K", [](L &t) { for (int j = 0; j < 2; j++) rotate(t.j[j], true, false, false, false); t.j[1].x_K = 1; }},  // (0 and 1 both mean the power-of-two rotation)
        {"shared x: x_hadk", [](L &t) { for (int j = 0; j < 2; j++) { t.j[j].k = 14336; rotate28(t.j[j], true); } t.j[1].x_hadk = HADK + 0x1000; }},
        {"K 28 beside K 1", [](L &t) { t.j[0].k = 14336; t.j[0].x = x_of(14336); rotate28(t.j[0], true); rotate(t.j[1], true, false, false, false); }},
        {"K 28 without x_hadk", [](L &t) { for (int j = 0; j < 2; j++) { t.j[j].k = 14336; rotate28(t.j[j], true); t.j[j].x_hadk = nullptr; } }},
        {"K 28 with x_f32", [](L &t) { for (int j = 0; j < 2; j++) { t.j[j].k = 14336; rotate28(t.j[j], true); t.j[j].x_f32 = x_of(14336, true); } }},
        {"K 28 at k 4096", [](L &t) { for (int j = 0; j < 2; j++) rotate28(t.j[j], true); }},
    };
    if constexpr (L::kTcq) {
        const std::vector<Rule> own = {
            {"c1 null", [](L &t) { t.j[0].c1 = nullptr; }},
            {"tlut null", [](L &t) { t.j[1].tlut = nullptr; }},
            {"c1 misaligned", [](L &t) { t.j[1].c1 = W1 + 2; }},
            {"split ROWS", [](L &t) { t.split = QPAL_SPLIT_ROWS; t.KV2 = 7; for (int j = 0; j < t.nj && j < 9; j++) t.j[j].c2 = W2; }},
            {"split COLS, c2 null", [](L &t) { t.split = QPAL_SPLIT_COLS; t.KV2 = 7; }},
            {"split COLS, KV2 != KV1 + 1", [](L &t) { t.split = QPAL_SPLIT_COLS; t.KV2 = 8; for (int j = 0; j < t.nj && j < 9; j++) t.j[j].c2 = W2; }},
            {"KV1 11", [](L &t) { t.KV1 = 11; }},
            {"kv2 without kv", [](L &t) { t.j[1].kv2 = 7; t.j[1].c2 = W2; }},
            {"kv2 without c2", [](L &t) { t.j[1].kv = 6; t.j[1].kv2 = 7; }},
            {"kv2 != kv + 1", [](L &t) { t.j[1].kv = 4; t.j[1].kv2 = 7; t.j[1].c2 = W2; }},
            {"mixed at n 9", [](L &t) { t.n = 9; t.j[1].kv = 4; }},
            {"mixed with x_had", [](L &t) { for (int j = 0; j < 2; j++) rotate(t.j[j], true, false, false, false); t.j[1].kv = 4; }},
            {"mixed with split COLS", [](L &t) { t.split = QPAL_SPLIT_COLS; t.KV2 = 7; for (int j = 0; j < 2; j++) t.j[j].c2 = W2; t.j[0].kv = 4; }},
            {"mixed, kv 9 at S 9", [](L &t) { t.j[0].kv = 9; }},
            {"mixed, kv 11", [](L &t) { t.j[0].kv = 11; }},
        };
        rules.insert(rules.end(), own.begin(), own.end());
    } else {
        const std::vector<Rule> own = {
            {"qweight null", [](L &t) { t.j[0].qweight = nullptr; }},
            {"lut null", [](L &t) { t.j[1].lut = nullptr; }},
            {"qweight misaligned", [](L &t) { t.j[1].qweight = W1 + 2; }},
            {"bits 9, vec 1", [](L &t) { t.bits = 9; }},
            {"vec 4", [](L &t) { t.vec = 4; }},
            {"bits * k % 64", [](L &t) { t.bits = 3; t.vec = 2; t.j[0].k = 32; t.j[0].x = x_of(32); }},
            {"128 KiB image at n 65", [](L &t) { t.bits = 12; t.vec = 2; t.n = 65; }},
            {"128 KiB image at n 128", [](L &t) { t.bits = 6; t.n = 128; }},
            {"K 28 beside a 32 KiB image", [](L &t) { t.bits = 8; t.vec = 2; for (int j = 0; j < 2; j++) { t.j[j].k = 14336; t.j[j].x = x_of(14336); rotate28(t.j[j], true); } }},
        };
        rules.insert(rules.end(), own.begin(), own.end());
    }
    int id = 0;
    const int nr = (int)rules.size();
    const int gaps[] = {1, 2, 3, 5, 8, 13, 21, 34};  // pairs (a, a + gap): every rule meets eight others, near and far in the order of the checks
    for (int a = -1; a < (g_reduced ? 0 : nr); a++)  // a = -1: the base launch itself (b = -1), then every rule on its own
        for (int b = a; b < nr; b++) {
            if (a >= 0 && !among(b - a, gaps)) continue;
            L t = launch_of<J>(2, 1, 1024, 4096);
            t.j[1].out = reinterpret_cast<float *>(OUT + sizeof(float) * 1024);
            begin(prefix, id++);
            if (a >= 0) { add(g_args, "[%s] ", rules[a].what); rules[a].apply(t); }
            if (b >= 0) { add(g_args, "[%s] ", rules[b].what); rules[b].apply(t); }
            end(call(t));
        }
}

// ---- seeded random launches: the variations above, combined
template <class J>
void sweep_random(const char *prefix, int cases) {
    const int ms[] = {32, 64, 96, 1024, 4096, 6144, 14336, 28672};
    const std::vector<std::vector<int>> kss = {{4096}, {4096, 14336}, {2048, 4096, 8192}, {64, 4096, 8192, 14336}, {2048}, {14336}};
    for (int id = 0; id < cases; id++) {
        Launch<J> t;
        t.n = chance(35) ? 1 : one_of(kNs);
        const bool rot = t.n == 1 && !g_reduced && chance(20);  // (the rotation needs k of 2048, 4096 or 14336)
        const int kdiv = plans_gemv(t.n) && !rot ? 16 : 1;
        if constexpr (Launch<J>::kTcq) {
            const auto &skv = kSKV[pick(7)];
            t.S = skv[0];
            t.KV1 = skv[1];
            if (chance(25)) { t.split = QPAL_SPLIT_COLS; t.KV2 = t.KV1 + 1; }
        } else {
            const auto &bv = kLut[pick(8)];
            t.bits = bv[0];
            t.vec = bv[1];
        }
        const std::vector<int> &ks = kss[pick((int)kss.size())];
        const int nj = 1 + pick(kMaxJobs);
        for (int j = 0; j < nj; j++) add_job(t, one_of(ms), ks[pick((int)ks.size())] / kdiv);
        lay_out(t, (Layout)pick(3));
        const int z = pick(3);
        const bool scales = chance(30), act = rot && chance(40), mixed = Launch<J>::kTcq && !t.split && chance(25);
        const int rbits = pick(16);
        for (int j = 0; j < nj; j++) {
            J &jb = t.j[j];
            jb.out_zeroed = z == 2 ? pick(2) : z;
            if (chance(20)) jb.accumulate = 1;
            if (scales) { jb.wscale = WSC + j * 0x10000; jb.oscale = one_of({0.f, 1.f, 0.25f}); }
            if (rot && jb.k == 14336) rotate28(jb, rbits & 1);
            else if (rot) rotate(jb, rbits & 1, rbits & 2, rbits & 4, rbits & 8);
            if (act && jb.m % 64 == 0 && !jb.accumulate && chance(60)) swiglu(jb, j, rbits & 1, chance(50));
            if constexpr (Launch<J>::kTcq)
                if (mixed && chance(60)) {
                    jb.kv = t.S == 9 ? 2 + pick(7) : t.S == 10 ? 8 + pick(3) : 9 + pick(2);
                    if (chance(30) && jb.k % 64 == 0) { jb.kv2 = jb.kv + 1; jb.c2 = W2 + (size_t)j * kJobStride; }
                }
        }
        if (chance(25)) { t.pz = PREZERO; t.pzb = 16L << pick(12); }
        begin(prefix, id);
        end(call(t));
    }
}

}  // namespace

int main(int argc, char **argv) {
    bool stats = false;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--reduced")) g_reduced = true;
        else if (!strcmp(argv[i], "--stats")) stats = true;
        else if (!strcmp(argv[i], "--show") && i + 1 < argc) {
            std::string ids = argv[++i];
            for (size_t p = 0; p <= ids.size();) {
                const size_t q = ids.find(',', p);
                g_show_ids.insert(ids.substr(p, q == std::string::npos ? q : q - p));
                if (q == std::string::npos) break;
                p = q + 1;
            }
        } else {
            fprintf(stderr, "usage: capi_trace [--reduced] [--stats] [--show id,id,...]\n");
            return 2;
        }
    }
    struct Sweep { const char *name; void (*run)(); };
    const Sweep sweeps[] = {
        {"tcq single", sweep_tcq_single},
        {"lut single", sweep_lut_single},
        {"tcq multi", [] { sweep_multi_shared<qpal_tcq_job>("mt"); }},
        {"lut multi", [] { sweep_multi_shared<qpal_lut_job>("ml"); }},
        {"tcq multi, own", sweep_tcq_multi_own},
        {"tcq invalid", [] { sweep_invalid<qpal_tcq_job>("it"); }},
        {"lut invalid", [] { sweep_invalid<qpal_lut_job>("il"); }},
        {"tcq random", [] { sweep_random<qpal_tcq_job>("rt", g_reduced ? 40 : 150); }},
        {"lut random", [] { sweep_random<qpal_lut_job>("rl", g_reduced ? 40 : 150); }},
    };
    for (const Sweep &sw : sweeps) {
        const clock_t t0 = clock();
        sw.run();
        if (stats) printf("# seconds %s %.2f\n", sw.name, (double)(clock() - t0) / CLOCKS_PER_SEC);
    }
    if (stats) {
        for (const auto &kv : g_launches) printf("# calls %s %d\n", kv.first.c_str(), kv.second);
        for (const auto &kv : g_codes) printf("# cases rc=%s %d\n", kv.first.c_str(), kv.second);
    }
    return 0;
}
