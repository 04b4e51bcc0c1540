// TEST INFRASTRUCTURE: the CPU emulation of every kernel family under AddressSanitizer and UBSan (tests/test_emu_sanitized.py,
// tests/hipemu/Makefile target `asan`, DESIGN.md "Sanitized emulation run").
//
// A stand-alone program: it includes the C-ABI header and calls exported functions only.  Each scenario runs in a context of its
// own (destroyed afterwards) with the profile on, prints one line, and passes if every call returned the code the scenario expects,
// what it reads back is finite, Sigma is symmetric to 1e-9 of max|Sigma|, and the slot statistics are what the scenario injected.
// Numerical parity is the pytest modules' business; this program exists so that the sanitizers see every index the kernels form at
// the sizes where one can run off the end.  At the end the profile spans of all scenarios are summed: each of the 32 spans of
// kProfNames must have run at least once.
//
// Kernels without a profile span of their own, and the scenarios that reach each:
//   k_merge_index / _align / _insert / _fuse     merge/two_maps_1024, merge/256_maps_40, merge/dup_and_range, fleet_slam/cap_and_max
//   k_ekf_export_map, k_fleet_export_maps        map_edit/ld63, map_edit/large (aslam_export_map); fleet_slam/cap_and_max (fleet merge)
//   k_relocalize, k_umap_clear_cross             reloc/localize, reloc/fleet (an uncertain-map fleet: every seat clears the cross strip)
//   k_rig_merge                                  rig/lists_128_129, rig/slam_step
//   k_render                                     image/synth_240x320, stream/ring_wrapped_once
//   k_clear_counts, k_prefix                     every image/* scenario
//   k_link_serial                                image/capacity_* (lds_nodes = 0: the serial cycle resolution)
//   corner refinement (inside the pose stage)    image/synth_240x320
//   k_ekf_win_gather, k_ekf_win_next_gather, k_ekf_win_thin, k_ekf_win_fix, k_ekf_win_next_fix
//                                                window/handover_split (ASLAM_WIN_NEXT_SPLIT: the four launches behind the hand-over)
//   k_ekf_predict                                image/synth_240x320 (aslam_add_encoder, then aslam_add_image)
//   k_confirm, k_confirm_reseed                  confirm/128, confirm/1 (span "confirm")
//   the uncertain-map strip in dynamic LDS       loc/uncertain_largest (1024 landmarks: the largest the call accepts)
#include "aruco_slam_hip.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr double WL = 2.0, WR = 2.3, DT = 1.0 / 30.0;
constexpr int kSpans = 32;

long long g_calls[kSpans];
const char* g_names[kSpans];
std::string g_fail;          // first failure of the running scenario
int g_failed = 0, g_run = 0;

void failf(const char* fmt, ...) {
    if (!g_fail.empty()) return;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_fail = buf;
}
#define CHECK(cond, ...) do { if (!(cond)) { failf(__VA_ARGS__); } } while (0)
#define EXPECT(call, code) do { const int r_ = (call); if (r_ != (code)) failf("%s:%d %s returned %d, expected %d", __FILE__, __LINE__, #call, r_, (int)(code)); } while (0)
#define OK(call) EXPECT(call, ASLAM_OK)

struct Rng {
    unsigned long long s;
    explicit Rng(unsigned long long seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) { next(); next(); }
    unsigned long long next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
    double uni(double a = 0, double b = 1) { return a + (b - a) * (double)(next() >> 11) / 9007199254740992.0; }
    double normal(double sd) { double u = 0; for (int i = 0; i < 12; i++) u += uni(); return (u - 6.0) * sd; }
    int below(int n) { return (int)(next() % (unsigned long long)n); }
};

double wrap_once(double a) { return a >= kPi ? a - 2 * kPi : a < -kPi ? a + 2 * kPi : a; }

aslam_init small_init(int cap, int max_landmarks, int batch) {
    aslam_init in;
    aslam_default_init(&in);
    in.max_rows = 64; in.max_cols = 64; in.max_batch = batch; in.persistent_waves = 4;
    in.max_landmarks = max_landmarks; in.max_updates_per_frame = cap;
    return in;
}

// a context with the profile on; its spans are added to the totals when it goes
struct Ctx {
    aslam_ctx* c = nullptr;
    explicit Ctx(const aslam_init& in) {
        const int r = aslam_create(&in, &c);
        if (r != ASLAM_OK) { failf("aslam_create returned %d", r); c = nullptr; return; }
        OK(aslam_profile_enable(c, 1));
        OK(aslam_profile_reset(c));
    }
    ~Ctx() {
        if (!c) return;
        const char* names[kSpans]; int calls[kSpans]; double ms[kSpans];
        const int n = aslam_profile_get(c, kSpans, names, calls, ms);
        CHECK(n == kSpans, "aslam_profile_get reports %d spans, the driver knows %d", n, kSpans);
        for (int i = 0; i < kSpans && i < n; i++) { g_names[i] = names[i]; g_calls[i] += calls[i]; }
        aslam_destroy(c);
    }
    operator aslam_ctx*() const { return c; }
    int calls(const char* name) const {
        const char* names[kSpans]; int calls[kSpans];
        const int n = aslam_profile_get(c, kSpans, names, calls, nullptr);
        for (int i = 0; i < n && i < kSpans; i++) if (!std::strcmp(names[i], name)) return calls[i];
        return -1;
    }
};

// mu (3 + 3L) and a dense symmetric positive definite Sigma (column-major N x N), heading just below pi so that the predict wraps
void seeded_state(Rng& g, int L, std::vector<double>& mu, std::vector<double>& S) {
    const int N = 3 + 3 * L, rank = 8;
    mu.assign(N, 0.0);
    mu[0] = 0.3; mu[1] = -0.2; mu[2] = kPi - 0.0009;
    for (int i = 0; i < L; i++) {
        const double ang = g.uni(0, 2 * kPi), rad = g.uni(1.0, 6.0);
        mu[3 + 3 * i] = rad * std::cos(ang); mu[4 + 3 * i] = rad * std::sin(ang); mu[5 + 3 * i] = g.uni(-kPi + 1e-3, kPi - 1e-3);
    }
    std::vector<double> A((size_t)N * rank);
    for (auto& a : A) a = g.normal(0.05);
    S.assign((size_t)N * N, 0.0);
    for (int i = 0; i < N; i++)
        for (int j = 0; j <= i; j++) {
            double s = 0;
            for (int k = 0; k < rank; k++) s += A[(size_t)i * rank + k] * A[(size_t)j * rank + k];
            S[(size_t)j * N + i] = S[(size_t)i * N + j] = s;
        }
    for (int i = 0; i < N; i++) S[(size_t)i * N + i] += g.uni(0.01, 0.05);
}

void predicted_pose(const double* p, double wl, double wr, double dt, double out[3]) {
    const double kl = 0.05, kr = 0.05, b = 0.09;
    const double dsl = kl * dt * wl, dsr = kr * dt * wr, dth = (dsr - dsl) / (2 * b), ds = 0.5 * (dsr + dsl), th = p[2] + 0.5 * dth;
    out[0] = p[0] + ds * std::cos(th); out[1] = p[1] + ds * std::sin(th); out[2] = wrap_once(p[2] + dth);
}

// the observation of landmark (lx, ly, lt) from `pose`, plus bounded noise, heading wrapped once
void observe(Rng& g, const double* lm, const double* pose, double noise, double z[3], double r[3]) {
    const double ct = std::cos(pose[2]), st = std::sin(pose[2]), dx = lm[0] - pose[0], dy = lm[1] - pose[1];
    z[0] = dx * ct + dy * st + g.uni(-noise, noise); z[1] = -dx * st + dy * ct + g.uni(-noise, noise); z[2] = wrap_once(lm[2] - pose[2] + g.uni(-noise, noise));
    for (int k = 0; k < 3; k++) r[k] = g.uni(0.02, 0.2);
}

struct ObsList {
    std::vector<int> ids, valid;
    std::vector<double> z, r;
    int n() const { return (int)ids.size(); }
    void add(int id, int v, const double* zz, const double* rr) { ids.push_back(id); valid.push_back(v); z.insert(z.end(), zz, zz + 3); r.insert(r.end(), rr, rr + 3); }
    int inject(aslam_ctx* c, int slot) const { return aslam_debug_inject_observations(c, slot, n(), ids.data(), valid.data(), z.data(), r.data()); }
};

bool all_finite(const std::vector<double>& v) { for (double x : v) if (!std::isfinite(x)) return false; return true; }

// reads the state back: finite, Sigma symmetric to 1e-9 of max|Sigma|; returns L
int check_state(aslam_ctx* c, int expect_L, std::vector<double>* mu_out = nullptr, std::vector<double>* S_out = nullptr) {
    int N = 0;
    OK(aslam_get_state(c, &N, nullptr, nullptr));
    if (N < 3) { failf("state size %d", N); return -1; }
    std::vector<double> mu(N), S((size_t)N * N);
    OK(aslam_get_state(c, &N, mu.data(), S.data()));
    CHECK(all_finite(mu), "mu is not finite");
    CHECK(all_finite(S), "Sigma is not finite");
    double mx = 0, asym = 0;
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) {
            mx = std::max(mx, std::fabs(S[(size_t)j * N + i]));
            asym = std::max(asym, std::fabs(S[(size_t)j * N + i] - S[(size_t)i * N + j]));
        }
    CHECK(asym <= 1e-9 * mx, "Sigma asymmetric by %g of max %g", asym, mx);
    if (expect_L >= 0) CHECK(N == 3 + 3 * expect_L, "state has N = %d, expected L = %d", N, expect_L);
    if (mu_out) *mu_out = mu;
    if (S_out) *S_out = S;
    return (N - 3) / 3;
}

void check_stats(aslam_ctx* c, int slot, int det, int app, int fused, int stat) {
    int st[4] = {-1, -1, -1, -1};
    OK(aslam_get_slot_ekf_stats(c, slot, 1, st));
    CHECK(st[0] == det && st[1] == app && st[2] == fused && st[3] == stat, "slot %d stats %d %d %d %d, expected %d %d %d %d", slot, st[0], st[1],
          st[2], st[3], det, app, fused, stat);
}

std::vector<int> spread_ids(int n, int stride = 7, int first = 3) {   // n distinct ids in [0, 1024)
    std::vector<int> ids(n);
    for (int i = 0; i < n; i++) ids[i] = (first + i * stride) % 1024;
    return ids;
}

void stage_two(aslam_ctx* c) {
    const double wl[2] = {0.0, WL}, wr[2] = {0.0, WR}, dt[2] = {0.0, DT};
    OK(aslam_stage_encoders(c, 0, 2, wl, wr, dt));
}

void scenario(const char* name, void (*fn)()) {
    g_fail.clear();
    std::printf("%-30s ", name);                       // the name first: a sanitizer report that ends the program follows it
    std::fflush(stdout);
    const auto t0 = std::chrono::steady_clock::now();
    fn();
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    g_run++;
    if (g_fail.empty()) std::printf("ok   %6.2f s\n", s);
    else { g_failed++; std::printf("FAIL %6.2f s  %s\n", s, g_fail.c_str()); }
    std::fflush(stdout);
}

// ---- per-frame SLAM chains (tests/test_ekf_sizes.py) ----------------------------------------------------------------------------
// one arming sample, then predict + m corrections of known landmarks at L = m landmarks, detection order reversed
void chain_case(int cap, int m, int L, int ML, const char* must_run) {
    Rng g(1000 * m + L + ML);
    std::vector<double> mu, S;
    seeded_state(g, L, mu, S);
    const std::vector<int> ids = spread_ids(L);
    Ctx c(small_init(cap, ML, 2));
    if (!c.c) return;
    OK(aslam_set_state(c, 3 + 3 * L, mu.data(), S.data(), ids.data()));
    stage_two(c);
    double pose[3];
    predicted_pose(mu.data(), WL, WR, DT, pose);
    ObsList o0, o1;
    for (int k = 0; k < m; k++) {                      // the first and the last landmark are always seen
        const int li = k == 0 ? L - 1 : k == m - 1 ? 0 : (L - 1 - k);
        double z[3], r[3];
        observe(g, &mu[3 + 3 * li], pose, 0.03, z, r);
        o1.add(ids[li], 1, z, r);
    }
    OK(o0.inject(c, 0));
    OK(o1.inject(c, 1));
    OK(aslam_run_staged(c, 0, 2, 2));
    OK(aslam_sync(c));
    check_stats(c, 1, m, 0, m, 0);
    check_state(c, L);
    CHECK(c.calls(must_run) > 0, "%s did not run", must_run);
}
void chain_fast() { chain_case(24, 24, 24, 24, "k_ekf_apply"); }
void chain_mid() { chain_case(64, 64, 64, 64, "k_ekf_mid64"); }
void chain_general() { chain_case(128, 128, 128, 128, "k_ekf_small"); }
// max_landmarks = 63, 42, 20 (mod 64): ld = 3 + 3 max_landmarks = 0, 1, 63 (mod 64)
void chain_fast_ld0() { chain_case(24, 24, 24, 63, "k_ekf_apply"); }
void chain_mid_ld1() { chain_case(64, 64, 64, 106, "k_ekf_mid64"); }
void chain_general_ld63() { chain_case(128, 128, 128, 148, "k_ekf_gather"); }
void chain_mid_33() { chain_case(64, 33, 33, 33, "k_ekf_mid64"); }

// 128 detections: known ids, one id several times, invalid entries and new ids, through the device's own plan
void chain_full_list() {
    const int L = 60, ML = 130, n_known = 50, n_dup = 5, n_invalid = 33, n_new = 128 - n_known - n_dup - n_invalid;
    Rng g(77);
    std::vector<double> mu, S;
    seeded_state(g, L, mu, S);
    const std::vector<int> ids = spread_ids(L + n_new);
    Ctx c(small_init(128, ML, 2));
    if (!c.c) return;
    OK(aslam_set_state(c, 3 + 3 * L, mu.data(), S.data(), ids.data()));
    stage_two(c);
    double pose[3], z[3], r[3];
    predicted_pose(mu.data(), WL, WR, DT, pose);
    ObsList o0, o1;
    std::vector<char> kinds;
    kinds.insert(kinds.end(), n_known, 'k'); kinds.insert(kinds.end(), n_dup, 'd'); kinds.insert(kinds.end(), n_invalid, 'i'); kinds.insert(kinds.end(), n_new, 'n');
    for (int k = 127; k > 0; k--) std::swap(kinds[k], kinds[g.below(k + 1)]);
    int known = 0, dup = 0, inv = 0, nw = 0;
    for (int k = 0; k < 128; k++) {
        if (kinds[k] == 'k') { observe(g, &mu[3 + 3 * known], pose, 0.03, z, r); o1.add(ids[known], 1, z, r); known++; }
        else if (kinds[k] == 'd') { observe(g, &mu[3 + 3 * 4], pose, 0.03, z, r); o1.add(ids[4], 1, z, r); dup++; }
        else if (kinds[k] == 'i') { observe(g, &mu[3], pose, 0.03, z, r); o1.add(inv % 2 ? -1 : ids[(inv * 3) % L], 0, z, r); inv++; }
        else {
            z[0] = g.uni(0.5, 2); z[1] = g.uni(-1, 1); z[2] = g.uni(-3, 3);
            for (double& x : r) x = g.uni(0.02, 0.2);
            o1.add(ids[L + nw], 1, z, r);
            nw++;
        }
    }
    CHECK(o1.n() == 128 && known == n_known && dup == n_dup && nw == n_new, "the list was built wrongly: %d known %d dup %d new %d", o1.n(), known, dup, nw);
    OK(o0.inject(c, 0));
    OK(o1.inject(c, 1));
    OK(aslam_run_staged(c, 0, 2, 2));
    OK(aslam_sync(c));
    check_stats(c, 1, 128, n_new, n_known + n_dup, 0);
    check_state(c, L + n_new);
    int n = 0;
    std::vector<int> oi(128), ox(128), oa(128);
    std::vector<double> oz(384), orr(384);
    OK(aslam_get_observations(c, &n, oi.data(), ox.data(), oa.data(), oz.data(), orr.data()));
    CHECK(n == 128 - inv, "%d observations popped, %d valid ones injected", n, 128 - inv);
    // a 129th observation is refused
    o1.add(5, 1, z, r);
    EXPECT(o1.inject(c, 1), ASLAM_E_INVALID);
}

// ---- augment (tests/test_plan_kernel.py) ----------------------------------------------------------------------------------------
void augment_case(int ML, int n_new, bool overflow, const std::vector<int>& ids) {
    Rng g(ML + n_new);
    Ctx c(small_init(24, ML, 2));
    if (!c.c) return;
    stage_two(c);
    ObsList o0, o1;
    for (int k = 0; k < n_new; k++) {
        double z[3] = {g.uni(0.5, 2), g.uni(-1, 1), g.uni(-3, 3)}, r[3] = {g.uni(0.02, 0.2), g.uni(0.02, 0.2), g.uni(0.02, 0.2)};
        o1.add(ids[k], 1, z, r);
    }
    OK(o0.inject(c, 0));
    OK(o1.inject(c, 1));
    OK(aslam_run_staged(c, 0, 2, 2));
    if (overflow) {
        EXPECT(aslam_sync(c), ASLAM_E_CAPACITY);
        const char* e = aslam_last_error(c);
        CHECK(e && std::strstr(e, "landmark"), "the overflow report does not name the landmarks: %s", e ? e : "(null)");
        check_state(c, -1);
        return;
    }
    OK(aslam_sync(c));
    check_stats(c, 1, n_new, n_new, 0, 0);
    check_state(c, n_new);
    int L = 0;
    std::vector<int> got(ML);
    OK(aslam_get_landmark_ids(c, &L, got.data()));
    CHECK(L == n_new, "%d landmark ids", L);
    std::vector<int> want(ids.begin(), ids.begin() + n_new);                       // the pop order is the queue's, not the list's
    got.resize(std::max(L, 0));
    std::sort(want.begin(), want.end()); std::sort(got.begin(), got.end());
    CHECK(got == want, "the landmark ids are not the injected ones");
}
void augment_fill() { augment_case(100, 100, false, spread_ids(100)); }
void augment_over_by_one() { augment_case(100, 101, true, spread_ids(101)); }
void augment_id_edges() { augment_case(9, 5, false, std::vector<int>{-1, 1023, 1024, 0, 5}); }

// ---- localization (tests/test_localize.py, test_uncertain_map.py, test_innovation_gate.py) -----------------------------------------
struct Map { std::vector<int> ids; std::vector<double> xyth, sig; };
Map make_map(Rng& g, int L) {
    Map m;
    m.ids = spread_ids(L, 1, L == 1024 ? 0 : 1);
    m.xyth.resize(3 * (size_t)L); m.sig.assign(9 * (size_t)L, 0.0);
    for (int i = 0; i < L; i++) {
        const double ang = g.uni(0, 2 * kPi), rad = g.uni(1.0, 6.0);
        m.xyth[3 * i] = rad * std::cos(ang); m.xyth[3 * i + 1] = rad * std::sin(ang); m.xyth[3 * i + 2] = g.uni(-3.1, 3.1);
        m.sig[9 * i] = g.uni(1e-4, 1e-3); m.sig[9 * i + 4] = g.uni(1e-4, 1e-3); m.sig[9 * i + 8] = g.uni(1e-4, 1e-3);
        m.sig[9 * i + 1] = m.sig[9 * i + 3] = 1e-5;
    }
    return m;
}
const double kPose0[3] = {0.1, -0.2, kPi - 0.003};
const double kSig0[9] = {0.02, 0.001, 0.0, 0.001, 0.03, -0.002, 0.0, -0.002, 0.01};

// a slot's list: m observations of map landmarks from kPose0 (first and last landmark among them), one far off (for the gate)
ObsList loc_list(Rng& g, const Map& m, int n_obs, bool outlier) {
    ObsList o;
    const int L = (int)m.ids.size();
    for (int k = 0; k < n_obs; k++) {
        const int li = k == 0 ? L - 1 : k == 1 ? 0 : (k * 5) % L;
        double z[3], r[3];
        observe(g, &m.xyth[3 * (size_t)li], kPose0, 0.01, z, r);
        if (outlier && k == n_obs / 2) { z[0] += 3.0; z[1] -= 2.0; }
        o.add(m.ids[li], 1, z, r);
    }
    return o;
}

// policy bits: 1 = uncertain map, 2 = innovation gate, 4 = consistent innovations
void loc_policy(int bits, int L, const int* counts, int n_slots) {
    Rng g(31 * bits + L);
    const Map m = make_map(g, L);
    Ctx c(small_init(24, L, n_slots));
    if (!c.c) return;
    if (bits & 2) { aslam_gate_params gp; aslam_default_gate_params(&gp); OK(aslam_set_innovation_gate(c, &gp)); }
    if (bits & 4) OK(aslam_set_consistent_innovations(c, 1));
    std::vector<double> wl(n_slots, 2.0), wr(n_slots, 2.5), dt(n_slots, 0.05);
    OK(aslam_stage_encoders(c, 0, n_slots, wl.data(), wr.data(), dt.data()));
    for (int s = 0; s < n_slots; s++) OK(loc_list(g, m, counts[s], (bits & 2) && counts[s] > 2).inject(c, s));
    if (bits & 1) OK(aslam_localize_begin_uncertain(c, L, m.ids.data(), m.xyth.data(), m.sig.data(), kPose0, kSig0));
    else OK(aslam_localize_begin(c, L, m.ids.data(), m.xyth.data(), kPose0, kSig0));
    for (int s = 0; s < n_slots; s++) {
        OK(aslam_run_staged(c, s, 1, 2));
        OK(aslam_sync(c));
        int st[4];
        OK(aslam_get_slot_ekf_stats(c, s, 1, st));
        CHECK(st[0] == counts[s] && st[1] == 0 && st[2] + st[3] <= counts[s], "slot %d stats %d %d %d %d for %d observations", s, st[0], st[1], st[2], st[3], counts[s]);
        if (!(bits & 2) && s > 0) CHECK(st[2] + st[3] == counts[s], "slot %d fused %d + %d of %d", s, st[2], st[3], counts[s]);
        if (bits & 2) {
            aslam_slot_health h;
            OK(aslam_get_slot_health(c, s, 1, &h));
            CHECK(h.attempted == h.accepted + h.rejected && std::isfinite(h.nis_sum) && std::isfinite(h.d2_max), "slot %d health %d %d %d", s, h.attempted, h.accepted, h.rejected);
            if (s > 0 && counts[s] > 2) CHECK(h.rejected >= 1, "slot %d: the far observation was not rejected", s);
        }
    }
    check_state(c, L);
    if (bits & 2) { aslam_track_health th; OK(aslam_get_track_health(c, &th)); CHECK(th.frames >= 1, "track frames %d", th.frames); }
    CHECK(c.calls("k_loc_steps") == n_slots, "k_loc_steps ran %d times", c.calls("k_loc_steps"));
    OK(aslam_localize_end(c));
}
const int kLocCounts[4] = {3, 0, 1, 128};
void loc_p0() { loc_policy(0, 128, kLocCounts, 4); }
void loc_p1() { loc_policy(1, 128, kLocCounts, 4); }
void loc_p2() { loc_policy(2, 128, kLocCounts, 4); }
void loc_p3() { loc_policy(3, 128, kLocCounts, 4); }
void loc_p4() { loc_policy(4, 128, kLocCounts, 4); }
void loc_p5() { loc_policy(5, 128, kLocCounts, 4); }
void loc_p6() { loc_policy(6, 128, kLocCounts, 4); }
void loc_p7() { loc_policy(7, 128, kLocCounts, 4); }
const int kLocOne[3] = {1, 0, 1};
void loc_L1() { loc_policy(0, 1, kLocOne, 3); }
void loc_L1_uncertain() { loc_policy(7, 1, kLocOne, 3); }
const int kLocBig[2] = {2, 128};
void loc_uncertain_largest() { loc_policy(1, 1024, kLocBig, 2); }     // kIdTableSize landmarks: the largest strip the dynamic LDS holds

// fleets of R robots with uneven slot counts, all in one staged call
void fleet_policy(int bits, int R, int L) {
    Rng g(57 * bits + R + L);
    const Map m = make_map(g, L);
    const int n_slots = R == 1 ? 3 : 6;
    Ctx c(small_init(24, L, n_slots));
    if (!c.c) return;
    if (bits & 2) { aslam_gate_params gp; aslam_default_gate_params(&gp); OK(aslam_set_innovation_gate(c, &gp)); }
    if (bits & 4) OK(aslam_set_consistent_innovations(c, 1));
    std::vector<aslam_camera> cams(R);
    std::vector<double> poses, sigs;
    for (int r = 0; r < R; r++) {
        std::memset(&cams[r], 0, sizeof cams[r]);
        const double K[9] = {300, 0, 32, 0, 300, 32, 0, 0, 1};
        std::memcpy(cams[r].K, K, sizeof K);
        cams[r].mount_x = 0.1 * r;
        poses.insert(poses.end(), kPose0, kPose0 + 3);
        sigs.insert(sigs.end(), kSig0, kSig0 + 9);
    }
    if (bits & 1) OK(aslam_fleet_begin_uncertain(c, R, cams.data(), L, m.ids.data(), m.xyth.data(), m.sig.data(), poses.data(), sigs.data()));
    else OK(aslam_fleet_begin(c, R, cams.data(), L, m.ids.data(), m.xyth.data(), poses.data(), sigs.data()));
    // slots: robot 0 has three (arming, none, 128 observations), robot 2 two (arming, one observation), robot 1 one (arming only).
    // The full list sits in the call's last slot: the slots' lists are one allocation, guarded where the last one ends.
    const int robot3[6] = {0, 2, 0, 1, 2, 0}, count3[6] = {2, 3, 0, 5, 1, 128};
    const int robot1[3] = {0, 0, 0}, count1[3] = {1, 0, 128};
    const int* robots = R == 1 ? robot1 : robot3;
    const int* counts = R == 1 ? count1 : count3;
    std::vector<double> wl(n_slots, 2.0), wr(n_slots, 2.5), dt(n_slots, 0.05);
    OK(aslam_stage_encoders(c, 0, n_slots, wl.data(), wr.data(), dt.data()));
    for (int s = 0; s < n_slots; s++) OK(loc_list(g, m, counts[s], (bits & 2) && counts[s] > 2).inject(c, s));
    OK(aslam_fleet_run_staged(c, 0, n_slots, robots, 2));
    OK(aslam_sync(c));
    for (int s = 0; s < n_slots; s++) {
        int st[4];
        OK(aslam_get_slot_ekf_stats(c, s, 1, st));
        CHECK(st[0] == counts[s] && st[1] == 0 && st[2] + st[3] <= counts[s], "slot %d stats %d %d %d %d for %d observations", s, st[0], st[1], st[2], st[3], counts[s]);
    }
    int nr = 0;
    std::vector<double> p(3 * R), sg(9 * R);
    OK(aslam_fleet_get_poses(c, R, &nr, p.data(), sg.data()));
    CHECK(nr == R && all_finite(p) && all_finite(sg), "fleet poses: %d robots or a non-finite value", nr);
    for (int r = 0; r < R; r++)
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) CHECK(std::fabs(sg[9 * r + 3 * i + j] - sg[9 * r + 3 * j + i]) <= 1e-9 * 0.03, "robot %d Sigma_xx asymmetric", r);
    if (bits & 1) {
        int Lc = 0;
        std::vector<double> cross(9 * (size_t)L);
        for (int r = 0; r < R; r++) { OK(aslam_fleet_get_cross(c, r, &Lc, cross.data())); CHECK(Lc == L && all_finite(cross), "robot %d cross strip", r); }
    }
    if (bits & 2) { std::vector<aslam_track_health> th(R); OK(aslam_fleet_get_health(c, R, &nr, th.data())); }
    CHECK(c.calls("k_fleet_steps") >= 1, "k_fleet_steps did not run");
    OK(aslam_fleet_end(c));
}
void fleet_p0() { fleet_policy(0, 3, 128); }
void fleet_p1() { fleet_policy(1, 3, 128); }
void fleet_p2() { fleet_policy(2, 3, 128); }
void fleet_p3() { fleet_policy(3, 3, 128); }
void fleet_p4() { fleet_policy(4, 3, 128); }
void fleet_p5() { fleet_policy(5, 3, 128); }
void fleet_p6() { fleet_policy(6, 3, 128); }
void fleet_p7() { fleet_policy(7, 3, 128); }
void fleet_one_robot() { fleet_policy(0, 1, 1); }
void fleet_one_robot_uncertain() { fleet_policy(7, 1, 1); }


// ---- windows (tests/test_ekf_window_flush.py, test_ekf_window_handover.py, test_slam_gate_windows.py, test_consistent_windows.py) ----
struct Group { int frames, lo, hi; };                      // `frames` frames that all see landmarks [lo, hi)
// mode bits: 1 = SLAM gate + gated windows, 2 = consistent innovations + consistent windows, 4 = a new id in the last frame
void window_case(int cap, int L, int ML, const std::vector<Group>& groups, int mode, int min_windows, const char* must_run) {
    Rng g(L * 131 + ML + mode);
    std::vector<double> mu, S;
    seeded_state(g, L, mu, S);
    const std::vector<int> ids = spread_ids(L + 1);
    int nfr = 1;
    for (const Group& gr : groups) nfr += gr.frames;
    Ctx c(small_init(cap, ML, nfr));
    if (!c.c) return;
    if (mode & 1) {
        aslam_gate_params gp; aslam_default_gate_params(&gp);
        OK(aslam_set_slam_gate(c, &gp));
        OK(aslam_set_slam_gate_windows(c, 1));
    }
    if (mode & 2) { OK(aslam_set_consistent_innovations(c, 1)); OK(aslam_set_consistent_windows(c, 1)); }
    OK(aslam_set_state(c, 3 + 3 * L, mu.data(), S.data(), ids.data()));
    std::vector<double> wl(nfr), wr(nfr), dt(nfr, 0.05);
    for (int f = 0; f < nfr; f++) { wl[f] = g.uni(1, 4); wr[f] = g.uni(1, 4); }
    dt[0] = 0.0;
    OK(aslam_stage_encoders(c, 0, nfr, wl.data(), wr.data(), dt.data()));
    OK(ObsList().inject(c, 0));
    double pose[3] = {mu[0], mu[1], mu[2]};
    std::vector<int> want_fused(nfr, 0), want_n(nfr, 0), want_new(nfr, 0);
    int f = 1;
    for (size_t gi = 0; gi < groups.size(); gi++)
        for (int k = 0; k < groups[gi].frames; k++, f++) {
            double nx[3];
            predicted_pose(pose, wl[f], wr[f], dt[f], nx);
            std::memcpy(pose, nx, sizeof nx);
            ObsList o;
            for (int li = groups[gi].hi - 1; li >= groups[gi].lo; li--) {
                double z[3], r[3];
                observe(g, &mu[3 + 3 * li], pose, 0.03, z, r);
                z[0] += (f & 1) ? 0.05 : -0.05;                                                      // never within 0.01 of the last sighting: no "stationary" no-op
                if ((mode & 1) && f == 3 && li == groups[gi].lo) { z[0] += 4.0; z[1] -= 3.0; }       // one sighting the gate must reject
                o.add(ids[li], 1, z, r);
            }
            want_n[f] = o.n(); want_fused[f] = o.n();
            if ((mode & 1) && f == 3) want_fused[f]--;
            if ((mode & 4) && f == nfr - 1) {
                double z[3] = {1.5, 0.2, 0.3}, r[3] = {0.05, 0.05, 0.05};
                o.add(ids[L], 1, z, r);
                want_n[f]++; want_new[f] = 1;
            }
            OK(o.inject(c, f));
        }
    OK(aslam_run_staged(c, 0, nfr, 2));
    OK(aslam_sync(c));
    for (int k = 1; k < nfr; k++) check_stats(c, k, want_n[k], want_new[k], want_fused[k], 0);
    check_state(c, L + ((mode & 4) ? 1 : 0));
    long long ps[4] = {0, 0, 0, 0};
    OK(aslam_get_plan_stats(c, ps));
    CHECK(ps[2] >= min_windows, "%lld windows formed (%lld frames in windows, %lld per frame), expected at least %d", ps[2], ps[0], ps[1], min_windows);
    CHECK(c.calls(must_run) > 0, "%s did not run", must_run);
    if (mode & 1) {
        aslam_slot_health h;
        OK(aslam_get_slot_health(c, 3, 1, &h));
        CHECK(h.rejected == 1 && h.attempted == want_n[3], "gated window frame 3: attempted %d rejected %d", h.attempted, h.rejected);
    }
}
void window_set(int n) { window_case(64, n, n + 3, {{9, 0, n}}, 0, 1, "k_ekf_win_step"); }
void window_20() { window_set(20); }
void window_21() { window_set(21); }
void window_41() { window_set(41); }
void window_42() { window_set(42); }
void window_63() { window_set(63); }
// 17 frames on 20 landmarks (closed rather than widened), 3 on 24 that overlap it, 3 on a disjoint 20: two hand-overs, 64 -> 128 -> 64 wide
void window_handover() { window_case(24, 54, 60, {{17, 0, 20}, {3, 10, 34}, {3, 34, 54}}, 0, 3, "k_ekf_win_next"); }
void window_handover_split() {
    setenv("ASLAM_WIN_NEXT_SPLIT", "1", 1);
    window_case(24, 54, 60, {{17, 0, 20}, {3, 10, 34}, {3, 34, 54}}, 0, 3, "k_ekf_win_next");
    unsetenv("ASLAM_WIN_NEXT_SPLIT");
}
void window_gated() { window_case(24, 12, 15, {{6, 0, 12}}, 1, 1, "k_ekf_win_gate_finish"); }
void window_consistent() { window_case(24, 12, 15, {{6, 0, 12}}, 2, 1, "k_ekf_win_step"); }
// a window on 5 landmarks of a state of 125 (ld = 63 mod 64 at max_landmarks 126), then a frame that appends one: the flush and the
// augment write the padded columns of Sigma far beyond the window's set
// the piece schedule (ASLAM_WIN_PIECE, read when the context is made): chains of 8 + 1 frames and the two launches that drain the replay
void window_pieces() {
    setenv("ASLAM_WIN_PIECE", "8", 1);
    window_case(64, 21, 24, {{9, 0, 21}}, 0, 1, "k_ekf_win_drain");
    unsetenv("ASLAM_WIN_PIECE");
}
void window_then_augment() { window_case(24, 125, 126, {{5, 60, 65}}, 4, 1, "k_ekf_win_flush"); }

// the SLAM gate on the per-frame chain (k_ekf_gate_finish)
void chain_gated() {
    const int L = 24;
    Rng g(404);
    std::vector<double> mu, S;
    seeded_state(g, L, mu, S);
    const std::vector<int> ids = spread_ids(L);
    Ctx c(small_init(24, L, 2));
    if (!c.c) return;
    aslam_gate_params gp; aslam_default_gate_params(&gp);
    OK(aslam_set_slam_gate(c, &gp));
    OK(aslam_set_state(c, 3 + 3 * L, mu.data(), S.data(), ids.data()));
    stage_two(c);
    double pose[3];
    predicted_pose(mu.data(), WL, WR, DT, pose);
    ObsList o;
    for (int li = 0; li < L; li++) {
        double z[3], r[3];
        observe(g, &mu[3 + 3 * li], pose, 0.03, z, r);
        if (li == 7) { z[0] += 5.0; z[1] += 5.0; }
        o.add(ids[li], 1, z, r);
    }
    OK(ObsList().inject(c, 0));
    OK(o.inject(c, 1));
    OK(aslam_run_staged(c, 0, 2, 2));
    OK(aslam_sync(c));
    check_stats(c, 1, L, 0, L - 1, 0);
    check_state(c, L);
    aslam_slot_health h;
    OK(aslam_get_slot_health(c, 1, 1, &h));
    CHECK(h.attempted == L && h.rejected == 1 && h.worst_id == ids[7], "gate: attempted %d rejected %d worst id %d", h.attempted, h.rejected, h.worst_id);
    CHECK(c.calls("k_ekf_gate_finish") > 0, "k_ekf_gate_finish did not run");
}

// ---- fleet SLAM (tests/test_fleet_slam_sizes.py) and the fleet merge (tests/test_merge_maps.py) --------------------------------------
void check_sigma(const char* what, int N, const std::vector<double>& mu, const std::vector<double>& S) {
    CHECK(all_finite(mu) && all_finite(S), "%s: a non-finite value", what);
    double mx = 0, asym = 0;
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) {
            mx = std::max(mx, std::fabs(S[(size_t)j * N + i]));
            asym = std::max(asym, std::fabs(S[(size_t)j * N + i] - S[(size_t)i * N + j]));
        }
    CHECK(asym <= 1e-9 * mx, "%s: Sigma asymmetric by %g of max %g", what, asym, mx);
}
aslam_camera plain_camera(double mount_x = 0, double yaw = 0) {
    aslam_camera cam;
    std::memset(&cam, 0, sizeof cam);
    const double K[9] = {100, 0, 48, 0, 100, 32, 0, 0, 1};
    std::memcpy(cam.K, K, sizeof K);
    cam.mount_x = mount_x; cam.mount_yaw = yaw;
    return cam;
}
ObsList reloc_list(Rng& g, const double* lm_xyth, const std::vector<int>& ids, int L, int n_obs, const double* true_pose, bool unknown_ids);
extern const double kTruePose[3];
void fleet_slam() {
    const int L = 24;                                   // robot 0: at the cap (24 corrections) and at max_landmarks; robot 1: three new landmarks
    Rng g(909);
    std::vector<double> mu, S;
    seeded_state(g, L, mu, S);
    const std::vector<int> ids = spread_ids(L);
    Ctx c(small_init(24, L, 4));
    if (!c.c) return;
    const aslam_camera cams[2] = {plain_camera(), plain_camera(0.1)};
    OK(aslam_fleet_slam_begin(c, 2, cams));
    OK(aslam_fleet_set_state(c, 0, 3 + 3 * L, mu.data(), S.data(), ids.data()));
    const double wl[4] = {0, 0, WL, WL}, wr[4] = {0, 0, WR, WR}, dt[4] = {0, 0, DT, DT};
    OK(aslam_stage_encoders(c, 0, 4, wl, wr, dt));
    double pose[3];
    predicted_pose(mu.data(), WL, WR, DT, pose);
    ObsList o2, o3;
    for (int li = L - 1; li >= 0; li--) { double z[3], r[3]; observe(g, &mu[3 + 3 * li], pose, 0.03, z, r); o2.add(ids[li], 1, z, r); }
    for (int k = 0; k < 3; k++) { double z[3] = {1.0 + k, 0.5 * k, 0.1 * k}, r[3] = {0.05, 0.05, 0.05}; o3.add(ids[k], 1, z, r); }
    OK(ObsList().inject(c, 0)); OK(ObsList().inject(c, 1)); OK(o2.inject(c, 2)); OK(o3.inject(c, 3));
    const int robots[4] = {0, 1, 0, 1};
    OK(aslam_fleet_run_staged(c, 0, 4, robots, 2));
    OK(aslam_sync(c));
    check_stats(c, 2, L, 0, L, 0);
    check_stats(c, 3, 3, 3, 0, 0);
    for (int r = 0; r < 2; r++) {
        int N = 0;
        OK(aslam_fleet_get_state(c, r, &N, nullptr, nullptr));
        CHECK(N == (r == 0 ? 3 + 3 * L : 12), "robot %d has N = %d", r, N);
        if (N < 3) return;
        std::vector<double> m(N), s((size_t)N * N);
        OK(aslam_fleet_get_state(c, r, &N, m.data(), s.data()));
        check_sigma("fleet SLAM robot", N, m, s);
    }
    // the fleet merge: robot 1's three landmarks carry ids robot 0 has too
    int n = 0;
    std::vector<int> mi(1024), seen(1024), round(2);
    std::vector<double> xy(3 * 1024), sg(9 * 1024), T(6);
    OK(aslam_fleet_merge_maps(c, 0, 2, 1024, &n, mi.data(), xy.data(), sg.data(), seen.data(), round.data(), T.data()));
    CHECK(n == L, "the merged map has %d entries, expected %d", n, L);
    xy.resize(3 * (size_t)std::max(n, 0)); sg.resize(9 * (size_t)std::max(n, 0));
    CHECK(all_finite(xy) && all_finite(sg) && all_finite(T), "fleet merge: a non-finite value");
    CHECK(round[0] == 0 && round[1] == 1, "fleet merge rounds %d %d", round[0], round[1]);
    // SLAM relocalization of the fleet: robot 0 against its own 24 landmarks (accepted), robot 1 from one sighting (refused)
    OK(reloc_list(g, &mu[3], ids, L, 1, kTruePose, false).inject(c, 2));
    OK(reloc_list(g, &mu[3], ids, L, 24, kTruePose, false).inject(c, 3));
    const int who[2] = {1, 0};
    aslam_relocalize_result rr[2];
    OK(aslam_fleet_slam_relocalize(c, 2, 2, who, nullptr, 1, rr));
    CHECK(rr[0].status != 0 && rr[1].status == 0, "fleet SLAM relocalization: status %d and %d", rr[0].status, rr[1].status);
    int removed[2] = {-1, -1};
    const int rm[2] = {ids[0], ids[L - 1]};
    OK(aslam_fleet_remove_landmarks(c, 2, rm, 0, nullptr, removed));
    CHECK(removed[0] == 2 && removed[1] == 1, "fleet removal took %d and %d landmarks", removed[0], removed[1]);
    OK(aslam_fleet_end(c));
}

// ---- map edit (tests/test_remove_landmarks.py): first, last, all; max_landmarks 20 gives ld = 63 ---------------------------------------
void map_edit_case(int L, int ML) {
    Rng g(L + 7 * ML);
    std::vector<double> mu, S;
    seeded_state(g, L, mu, S);
    const std::vector<int> ids = spread_ids(L);
    Ctx c(small_init(24, ML, 2));
    if (!c.c) return;
    OK(aslam_set_state(c, 3 + 3 * L, mu.data(), S.data(), ids.data()));
    std::vector<unsigned char> rec((size_t)ML * ASLAM_MAP_RECORD_BYTES);
    OK(aslam_export_map(c, rec.data(), 0));
    int removed = -1;
    OK(aslam_remove_landmarks(c, 1, &ids[0], &removed));
    CHECK(removed == 1, "removing the first landmark removed %d", removed);
    check_state(c, L - 1);
    OK(aslam_remove_landmarks(c, 1, &ids[L - 1], &removed));
    CHECK(removed == 1, "removing the last landmark removed %d", removed);
    std::vector<double> mu2, S2;
    check_state(c, L - 2, &mu2, &S2);
    for (int i = 0; i < 3 * (L - 2); i++) CHECK(mu2[3 + i] == mu[6 + i], "kept landmark entry %d changed", i);
    OK(aslam_remove_landmarks(c, L, ids.data(), &removed));
    CHECK(removed == L - 2, "removing all landmarks removed %d", removed);
    check_state(c, 0);
    const int bad = 1024;
    EXPECT(aslam_remove_landmarks(c, 1, &bad, &removed), ASLAM_E_INVALID);
    OK(aslam_export_map(c, rec.data(), 0));
    CHECK(c.calls("k_map_plan") >= 3 && c.calls("k_map_cols") >= 1 && c.calls("k_map_rows") >= 1, "the map edit kernels did not all run");
}
void map_edit_ld63() { map_edit_case(20, 20); }
void map_edit_large() { map_edit_case(100, 128); }

// ---- merge (tests/test_merge_maps.py) ----------------------------------------------------------------------------------------------
struct MapRecord { int32_t id, index; double x, y, th; double S[9]; };
static_assert(sizeof(MapRecord) == ASLAM_MAP_RECORD_BYTES, "the map record layout");
void merge_case(int n_maps, int per_map, const std::vector<int>& id_of_pos, int expect_n) {
    Rng g(n_maps * 1000 + per_map);
    std::vector<double> base(3 * 1025);
    for (int i = 0; i < 1025; i++) { base[3 * i] = g.uni(-5, 5); base[3 * i + 1] = g.uni(-5, 5); base[3 * i + 2] = g.uni(-3.1, 3.1); }
    std::vector<MapRecord> rec((size_t)n_maps * per_map);
    for (int m = 0; m < n_maps; m++) {
        const double phi = 0.3 * m - 1.0, tx = 0.5 * m, ty = -0.25 * m, cp = std::cos(phi), sp = std::sin(phi);
        for (int k = 0; k < per_map; k++) {
            MapRecord& r = rec[(size_t)m * per_map + k];
            std::memset(&r, 0, sizeof r);
            r.id = id_of_pos[k]; r.index = k;
            const double* b = &base[3 * (size_t)std::min(std::max(r.id, 0), 1024)];
            r.x = cp * b[0] - sp * b[1] + tx + g.normal(0.002); r.y = sp * b[0] + cp * b[1] + ty + g.normal(0.002); r.th = wrap_once(b[2] + phi);
            r.S[0] = g.uni(1e-4, 1e-3); r.S[4] = g.uni(1e-4, 1e-3); r.S[8] = g.uni(1e-4, 1e-3); r.S[1] = r.S[3] = 2e-5;
        }
    }
    Ctx c(small_init(24, 8, 1));
    if (!c.c) return;
    int n = -1;
    std::vector<int> ids(1024), seen(1024), round(n_maps);
    std::vector<double> xy(3 * 1024), sg(9 * 1024), T(3 * (size_t)n_maps);
    OK(aslam_merge_map_records(c, rec.data(), 0, n_maps, per_map, 0, 2, 1024, &n, ids.data(), xy.data(), sg.data(), seen.data(), round.data(), T.data()));
    CHECK(n == expect_n, "the merged map has %d entries, expected %d", n, expect_n);
    xy.resize(3 * (size_t)std::max(n, 0)); sg.resize(9 * (size_t)std::max(n, 0));
    CHECK(all_finite(xy) && all_finite(sg) && all_finite(T), "merge: a non-finite value");
    for (int m = 0; m < n_maps; m++) CHECK(round[m] == (m == 0 ? 0 : 1), "map %d aligned in round %d", m, round[m]);
    for (int k = 0; k < n; k++) CHECK(seen[k] == n_maps, "id %d fused from %d maps of %d", ids[k], seen[k], n_maps);
    long long bytes = 0;
    OK(aslam_merge_scratch_bytes(c, &bytes));
    CHECK(bytes > 0, "merge scratch %lld bytes", bytes);
    EXPECT(aslam_merge_map_records(c, rec.data(), 0, n_maps, 1025, 0, 2, 1024, &n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), ASLAM_E_INVALID);
}
std::vector<int> iota_ids(int n) { std::vector<int> v(n); for (int i = 0; i < n; i++) v[i] = i; return v; }
void merge_two_1024() { merge_case(2, 1024, iota_ids(1024), 1024); }
void merge_256_40() { std::vector<int> v = iota_ids(40); for (int& x : v) x = 1023 - 25 * x; merge_case(256, 40, v, 40); }
void merge_dup_range() { merge_case(3, 9, std::vector<int>{5, 5, -1, 1024, 7, 1023, 0, 7, 2000000000}, 4); }

// ---- relocalize, SLAM relocalize, landmark confirmation ------------------------------------------------------------------------------
ObsList reloc_list(Rng& g, const double* lm_xyth, const std::vector<int>& ids, int L, int n_obs, const double* true_pose, bool unknown_ids) {
    ObsList o;
    for (int k = 0; k < n_obs; k++) {
        const int li = k == 0 ? L - 1 : k == 1 ? 0 : (k * 3) % L;
        double z[3], r[3];
        observe(g, &lm_xyth[3 * (size_t)li], true_pose, 0.005, z, r);
        o.add(unknown_ids ? 1000 + (k % 24) : ids[li], 1, z, r);
    }
    return o;
}
extern const double kTruePose[3] = {1.4, 0.7, -2.0};
void check_reloc(const aslam_relocalize_result& r, int status, int n_obs) {
    CHECK(r.status == status, "relocalize status %d, expected %d (%d candidates, %d inliers)", r.status, status, r.n_candidates, r.n_inliers);
    for (double v : r.pose) CHECK(std::isfinite(v), "relocalize pose not finite");
    for (double v : r.sigma) CHECK(std::isfinite(v), "relocalize sigma not finite");
    if (status == 0) {
        CHECK(r.n_inliers == n_obs && r.n_candidates == n_obs, "relocalize: %d candidates, %d inliers of %d", r.n_candidates, r.n_inliers, n_obs);
        CHECK(std::fabs(r.pose[0] - kTruePose[0]) < 0.1 && std::fabs(r.pose[1] - kTruePose[1]) < 0.1 && std::fabs(wrap_once(r.pose[2] - kTruePose[2])) < 0.1,
              "relocalized to %g %g %g", r.pose[0], r.pose[1], r.pose[2]);
    }
}
void reloc_localize() {
    const int L = 128;
    Rng g(515);
    const Map m = make_map(g, L);
    Ctx c(small_init(24, L, 4));
    if (!c.c) return;
    OK(ObsList().inject(c, 0));
    OK(reloc_list(g, m.xyth.data(), m.ids, L, 1, kTruePose, false).inject(c, 1));        // refused: one candidate, two needed
    OK(reloc_list(g, m.xyth.data(), m.ids, L, 128, kTruePose, true).inject(c, 2));       // refused: no id of the map
    OK(reloc_list(g, m.xyth.data(), m.ids, L, 128, kTruePose, false).inject(c, 3));      // accepted, 128, in the last slot
    OK(aslam_localize_begin(c, L, m.ids.data(), m.xyth.data(), kPose0, kSig0));
    aslam_relocalize_result r;
    OK(aslam_relocalize(c, 3, nullptr, 0, &r)); check_reloc(r, 0, 128);
    OK(aslam_relocalize(c, 1, nullptr, 1, &r)); check_reloc(r, 2, 1);
    OK(aslam_relocalize(c, 2, nullptr, 1, &r)); check_reloc(r, 1, 0);
    OK(aslam_relocalize(c, 0, nullptr, 1, &r)); check_reloc(r, 1, 0);
    aslam_relocalize_params p; aslam_default_relocalize_params(&p); p.min_inliers = 1;
    OK(aslam_relocalize(c, 1, &p, 1, &r)); check_reloc(r, 0, 1);                         // accepted, list length 1
    check_state(c, L);
    EXPECT(aslam_relocalize(c, 4, nullptr, 0, &r), ASLAM_E_INVALID);
}
void reloc_fleet() {
    const int L = 128, R = 3;
    Rng g(616);
    const Map m = make_map(g, L);
    Ctx c(small_init(24, L, 3));
    if (!c.c) return;
    aslam_camera cams[R]; std::vector<double> poses, sigs;
    for (int r = 0; r < R; r++) { cams[r] = plain_camera(); poses.insert(poses.end(), kPose0, kPose0 + 3); sigs.insert(sigs.end(), kSig0, kSig0 + 9); }
    OK(aslam_fleet_begin_uncertain(c, R, cams, L, m.ids.data(), m.xyth.data(), m.sig.data(), poses.data(), sigs.data()));
    OK(ObsList().inject(c, 0));
    OK(reloc_list(g, m.xyth.data(), m.ids, L, 1, kTruePose, false).inject(c, 1));
    OK(reloc_list(g, m.xyth.data(), m.ids, L, 128, kTruePose, false).inject(c, 2));
    const int robots[3] = {2, 0, 1};
    aslam_relocalize_result out[3];
    OK(aslam_fleet_relocalize(c, 0, 3, robots, nullptr, 1, out));
    check_reloc(out[0], 1, 0); check_reloc(out[1], 2, 1); check_reloc(out[2], 0, 128);
    int nr = 0; std::vector<double> p(3 * R), sg(9 * R);
    OK(aslam_fleet_get_poses(c, R, &nr, p.data(), sg.data()));
    CHECK(all_finite(p) && all_finite(sg), "fleet poses after the seat");
}
void reloc_slam() {
    const int L = 128;
    Rng g(717);
    std::vector<double> mu, S;
    seeded_state(g, L, mu, S);
    for (double& v : S) v *= 0.01;
    const std::vector<int> ids = spread_ids(L);
    Ctx c(small_init(24, L, 3));
    if (!c.c) return;
    OK(aslam_set_state(c, 3 + 3 * L, mu.data(), S.data(), ids.data()));
    OK(reloc_list(g, &mu[3], ids, L, 128, kTruePose, false).inject(c, 0));
    OK(reloc_list(g, &mu[3], ids, L, 1, kTruePose, false).inject(c, 1));
    OK(reloc_list(g, &mu[3], ids, L, 128, kTruePose, true).inject(c, 2));
    aslam_relocalize_result r;
    OK(aslam_slam_relocalize(c, 1, nullptr, 1, &r)); check_reloc(r, 2, 1);
    OK(aslam_slam_relocalize(c, 2, nullptr, 1, &r)); check_reloc(r, 1, 0);
    OK(aslam_slam_relocalize(c, 0, nullptr, 1, &r)); check_reloc(r, 0, 128);
    check_state(c, L);
    aslam_relocalize_params p; aslam_default_relocalize_params(&p); p.min_inliers = 1;
    OK(aslam_slam_relocalize(c, 1, &p, 1, &r)); check_reloc(r, 0, 1);
    check_state(c, L);
    CHECK(c.calls("k_slam_reloc_solve") >= 4 && c.calls("k_slam_reloc_seat") >= 1, "the SLAM relocalization kernels did not run");
}
void confirm_case(int n_obs) {
    Rng g(818 + n_obs);
    Ctx c(small_init(128, 130, 3));
    if (!c.c) return;
    const aslam_confirm_params cp = {2, 10};
    OK(aslam_set_landmark_confirmation(c, &cp));
    const double wl[3] = {0, WL, WL}, wr[3] = {0, WR, WR}, dt[3] = {0, DT, DT};
    OK(aslam_stage_encoders(c, 0, 3, wl, wr, dt));
    const std::vector<int> ids = spread_ids(128);
    for (int s = 0; s < 3; s++) {
        ObsList o;
        for (int k = 0; k < n_obs; k++) {
            double z[3] = {g.uni(0.5, 2), g.uni(-1, 1), g.uni(-3, 3)}, r[3] = {0.05, 0.05, 0.05};
            o.add(s == 2 && k == 0 ? 1023 : ids[k], 1, z, r);           // refused in slot 2: a first sighting of id 1023 is withheld
        }
        OK(o.inject(c, s));
    }
    OK(aslam_run_staged(c, 0, 3, 2));
    OK(aslam_sync(c));
    aslam_slot_confirm sc[3];
    OK(aslam_get_slot_confirm(c, 0, 3, sc));
    CHECK(sc[0].judged == n_obs && sc[0].withheld == n_obs && sc[0].promoted == 0, "slot 0: judged %d withheld %d promoted %d", sc[0].judged, sc[0].withheld, sc[0].promoted);
    CHECK(sc[1].promoted == n_obs && sc[1].withheld == 0, "slot 1: withheld %d promoted %d", sc[1].withheld, sc[1].promoted);
    CHECK(sc[2].withheld == 1 && (sc[2].withheld_mask[0] & 1u), "slot 2: withheld %d mask %x", sc[2].withheld, sc[2].withheld_mask[0]);
    check_stats(c, 1, n_obs, n_obs, 0, 0);
    check_state(c, n_obs);
    int nt = 0, tid[4], tc[4], ta[4];
    OK(aslam_get_tentative(c, 4, &nt, tid, tc, ta));
    CHECK(nt == 1 && tid[0] == 1023 && tc[0] == 1, "%d tentative ids", nt);
    CHECK(c.calls("confirm") > 0, "the confirmation stage did not run");
}
void confirm_128() { confirm_case(128); }
void confirm_1() { confirm_case(1); }

// ---- rig (tests/test_camera_rig.py) ------------------------------------------------------------------------------------------------------
void rig_lists() {
    aslam_init in = small_init(24, 300, 2);
    in.max_cols = 96;
    Ctx c(in);
    if (!c.c) return;
    const aslam_camera cams[2] = {plain_camera(), plain_camera(0, kPi)};
    OK(aslam_set_camera_rig(c, 2, cams));
    const double z2[2] = {0, 0}, dt[2] = {0.1, 0.1};
    OK(aslam_stage_encoders(c, 0, 2, z2, z2, dt));
    auto inject = [&](int n0, int n1, int base) {
        const int lo[2] = {base, base + 100}, n[2] = {n0, n1};
        for (int s = 0; s < 2; s++) {
            ObsList o;
            for (int k = 0; k < n[s]; k++) { const int id = lo[s] + k; double z[3] = {1.0 + 0.01 * id, 0.001 * id, 0}, r[3] = {0.02, 0.02, 0.02}; o.add(id, 1, z, r); }
            OK(o.inject(c, s));
        }
    };
    int st[4];
    inject(64, 64, 0);                                   // exactly kMarkerMax
    OK(aslam_run_staged_rig(c, 0, 1, 2));
    OK(aslam_sync(c));
    OK(aslam_get_rig_step_ekf_stats(c, 0, 1, st));
    CHECK(st[0] == 128 && st[1] == 128 && st[2] == 0 && st[3] == 0, "rig step stats %d %d %d %d", st[0], st[1], st[2], st[3]);
    inject(70, 59, 300);                                 // 129: the merged list overflows by one
    OK(aslam_run_staged_rig(c, 0, 1, 2));
    EXPECT(aslam_sync(c), ASLAM_E_CAPACITY);
    OK(aslam_get_rig_step_ekf_stats(c, 0, 1, st));
    CHECK(st[0] == 128 && st[1] == 128, "rig step stats after the overflow %d %d %d %d", st[0], st[1], st[2], st[3]);
    check_state(c, 256);
    int n = 0; std::vector<int> oi(128), ox(128), oa(128), oc(128); std::vector<double> oz(384), orr(384);
    OK(aslam_get_rig_observations(c, &n, oi.data(), ox.data(), oa.data(), oc.data(), oz.data(), orr.data()));
}
void rig_slam_step() {
    const int L = 20;
    Rng g(929);
    std::vector<double> mu, S;
    seeded_state(g, L, mu, S);
    const std::vector<int> ids = spread_ids(L);
    Ctx c(small_init(24, L + 2, 4));
    if (!c.c) return;
    const aslam_camera cams[2] = {plain_camera(), plain_camera(0, 1.0)};
    OK(aslam_set_camera_rig(c, 2, cams));
    OK(aslam_set_state(c, 3 + 3 * L, mu.data(), S.data(), ids.data()));
    const double wl[4] = {0, 0, WL, WL}, wr[4] = {0, 0, WR, WR}, dt[4] = {0, 0, DT, DT};
    OK(aslam_stage_encoders(c, 0, 4, wl, wr, dt));
    double pose[3];
    predicted_pose(mu.data(), WL, WR, DT, pose);
    ObsList a, b;
    for (int li = 0; li < L; li++) { double z[3], r[3]; observe(g, &mu[3 + 3 * li], pose, 0.03, z, r); (li % 2 ? a : b).add(ids[li], 1, z, r); }
    OK(ObsList().inject(c, 0)); OK(ObsList().inject(c, 1)); OK(a.inject(c, 2)); OK(b.inject(c, 3));
    OK(aslam_run_staged_rig(c, 0, 2, 2));
    OK(aslam_sync(c));
    int st[4];
    OK(aslam_get_rig_step_ekf_stats(c, 1, 1, st));
    CHECK(st[0] == L && st[1] == 0 && st[2] == L, "rig SLAM step stats %d %d %d %d", st[0], st[1], st[2], st[3]);
    check_state(c, L);
}


// ---- detection and pose on images ------------------------------------------------------------------------------------------------------
struct Image {                                         // the last row is cols * channels bytes long: the buffer ends where the frame ends
    int rows, cols, ch; size_t step;
    std::vector<uint8_t> px;
    Image(int r, int c, int channels, size_t pad) : rows(r), cols(c), ch(channels), step((size_t)c * channels + pad), px((size_t)(r - 1) * step + (size_t)c * channels, 255) {}
    void set(int y, int x, uint8_t v) { if (y >= 0 && y < rows && x >= 0 && x < cols) for (int k = 0; k < ch; k++) px[(size_t)y * step + (size_t)x * ch + k] = v; }
    void rect(int x0, int y0, int w, int h, uint8_t v) { for (int y = y0; y < y0 + h; y++) for (int x = x0; x < x0 + w; x++) set(y, x, v); }
    void ring(int x0, int y0, int w, int h) { rect(x0, y0, w, 1, 0); rect(x0, y0 + h - 1, w, 1, 0); rect(x0, y0, 1, h, 0); rect(x0 + w - 1, y0, 1, h, 0); }
};
const double kCamK[9] = {250, 0, 160, 0, 250, 120, 0, 0, 1};
const double kCamD[5] = {0, 0, 0, 0, 0};

// frames of 1 x 1, 1 x 70, 70 x 1, 33 x 65 and 97 x 129 with a row step that is no multiple of 4 (the byte path of k_threshold)
void image_small(int channels) {
    aslam_init in = small_init(24, 16, 1);
    in.max_rows = 97; in.max_cols = 129;
    Ctx c(in);
    if (!c.c) return;
    OK(aslam_set_camera(c, kCamK, kCamD, 5));
    const int shapes[5][2] = {{1, 1}, {1, 70}, {70, 1}, {33, 65}, {97, 129}};
    for (const auto& sh : shapes) {
        const size_t row = (size_t)sh[1] * channels;
        Image im(sh[0], sh[1], channels, (row + 3) % 4 == 0 ? 2 : 3);          // row + pad is never a multiple of 4
        im.rect(sh[1] / 4, sh[0] / 4, sh[1] / 2, sh[0] / 2, 0);              // a dark block, a ring at the frame's edge and one inside
        im.ring(0, 0, sh[1], sh[0]);
        im.rect(sh[1] / 4 + 3, sh[0] / 4 + 3, sh[1] / 2 - 6, sh[0] / 2 - 6, 255);
        int count = -1, ids[8]; float corners[64]; double rv[24], tv[24];
        OK(aslam_detect_batch(c, im.px.data(), 1, sh[0], sh[1], channels, im.step, im.px.size(), 8, &count, ids, corners, rv, tv));
        CHECK(count == 0, "%d x %d: %d markers in a frame without one", sh[0], sh[1], count);
        unsigned fc[6];
        OK(aslam_debug_get_frame_counts(c, 0, fc));
    }
    CHECK(c.calls("k_threshold") >= 5, "k_threshold ran %d times", c.calls("k_threshold"));
}
void image_small_gray() { image_small(1); }
void image_small_bgr() { image_small(3); }

void marker_poses(double tz, double* poses /* 4 x 12 */) {
    const double xs[4] = {-0.42, 0.42, -0.42, 0.42}, ys[4] = {-0.27, -0.27, 0.27, 0.27}, psi[4] = {0.2, -0.3, 0.1, -0.15};
    for (int k = 0; k < 4; k++) {
        const double c = std::cos(psi[k]), s = std::sin(psi[k]);
        const double R[9] = {c, 0, -s, 0, -1, 0, -s, 0, -c};
        std::memcpy(poses + 12 * k, R, sizeof R);
        poses[12 * k + 9] = xs[k]; poses[12 * k + 10] = ys[k]; poses[12 * k + 11] = tz;
    }
}
// one 240 x 320 frame with four markers: detect_batch, the staged path with the EKF, then corner refinement, the ambiguity check and
// the observation covariance switched on, once each
void image_synth() {
    aslam_init in = small_init(24, 16, 2);
    in.max_rows = 240; in.max_cols = 320;
    Ctx c(in);
    if (!c.c) return;
    OK(aslam_set_camera(c, kCamK, kCamD, 5));
    const int mids[4] = {7, 100, 513, 1023};
    double poses[48];
    std::vector<uint8_t> host((size_t)240 * 320);
    marker_poses(1.6, poses);
    OK(aslam_synth_render(c, 0, 240, 320, kCamK, 4, mids, poses, 0.27, 200, 2, 1, 1, host.data()));
    int count = -1, ids[8]; float corners[64]; double rv[24], tv[24];
    OK(aslam_detect_batch(c, host.data(), 1, 240, 320, 1, 320, host.size(), 8, &count, ids, corners, rv, tv));
    CHECK(count == 4, "detect_batch found %d of 4 markers", count);
    for (int k = 0; k < count && k < 4; k++) CHECK(std::isfinite(tv[3 * k + 2]) && std::fabs(tv[3 * k + 2] - 1.6) < 0.2, "marker %d at depth %g", ids[k], tv[3 * k + 2]);
    OK(aslam_synth_render(c, 0, 240, 320, kCamK, 4, mids, poses, 0.27, 200, 2, 1, 1, nullptr));
    marker_poses(1.75, poses);
    OK(aslam_synth_render(c, 1, 240, 320, kCamK, 4, mids, poses, 0.27, 200, 2, 2, 1, nullptr));
    const double wl[2] = {0, WL}, wr[2] = {0, WR}, dt[2] = {0, DT};
    OK(aslam_stage_encoders(c, 0, 2, wl, wr, dt));
    OK(aslam_run_staged(c, 0, 2, 1));
    OK(aslam_sync(c));
    check_stats(c, 0, 4, 4, 0, 0);
    check_stats(c, 1, 4, 0, 4, 0);
    check_state(c, 4);
    aslam_detector_params dp;
    aslam_default_detector_params(&dp);
    dp.doCornerRefinement = 1;
    OK(aslam_set_detector_params(c, &dp));
    OK(aslam_run_staged(c, 0, 2, 0));
    OK(aslam_sync(c));
    int M = 0;
    OK(aslam_get_slot_detections(c, 1, &M, ids, corners, rv, tv));
    CHECK(M == 4, "with corner refinement: %d markers", M);
    for (int k = 0; k < 8 * std::min(M, 4); k++) CHECK(std::isfinite(corners[k]), "refined corner not finite");
    dp.doCornerRefinement = 0;
    OK(aslam_set_detector_params(c, &dp));
    aslam_pose_ambiguity_params ap;
    aslam_default_pose_ambiguity_params(&ap);
    OK(aslam_set_pose_ambiguity(c, &ap));
    OK(aslam_run_staged(c, 0, 2, 0));
    OK(aslam_sync(c));
    int n = 0; aslam_pose_ambiguity amb[8]; aslam_slot_pose_ambiguity asum;
    OK(aslam_get_slot_pose_ambiguity(c, 1, 8, &n, amb, &asum));
    CHECK(n == 4 && asum.checked == 4, "ambiguity check: %d records, %d checked", n, asum.checked);
    for (int k = 0; k < std::min(n, 4); k++) CHECK(std::isfinite(amb[k].rms) && std::isfinite(amb[k].rms_alt) && std::isfinite(amb[k].dtheta), "ambiguity record %d not finite", k);
    OK(aslam_set_pose_ambiguity(c, nullptr));
    aslam_obs_covariance_params op;
    aslam_default_obs_covariance_params(&op);
    OK(aslam_set_observation_covariance(c, &op));
    OK(aslam_run_staged(c, 0, 2, 0));
    OK(aslam_sync(c));
    aslam_obs_covariance cov[8]; aslam_slot_obs_covariance csum;
    OK(aslam_get_slot_obs_covariance(c, 1, 8, &n, cov, &csum));
    CHECK(n == 4 && csum.checked == 4 && csum.degenerate == 0, "observation covariance: %d records, %d checked, %d degenerate", n, csum.checked, csum.degenerate);
    for (int k = 0; k < std::min(n, 4); k++)
        for (int i = 0; i < 9; i++) CHECK(std::isfinite(cov[k].cov[i]) && cov[k].cov[i] == cov[k].cov[3 * (i % 3) + i / 3], "covariance record %d", k);
    CHECK(c.calls("k_pose_alt") >= 1 && c.calls("k_pose_cov") >= 1 && c.calls("k_identify") >= 3, "a pose-stage kernel did not run");
    // the reference's own entry points: an encoder sample (the predict-only kernel), then one borrowed image
    OK(aslam_add_encoder(c, WL, WR, 10.0));
    OK(aslam_add_encoder(c, WL, WR, 10.05));
    OK(aslam_add_image(c, host.data(), 240, 320, 1, 320));
    check_state(c, 4);
}

// the three capacity overflows of tests/test_contours_kernel.py: start candidates, contours, points; both forms of the link
void contour_capacity(unsigned starts, unsigned contours, unsigned points, int kind, double min_rate, double max_rate) {
    const int rows = 40, cols = 72;
    aslam_init in = small_init(24, 16, 1);
    in.max_rows = rows; in.max_cols = cols;
    in.cap_starts_per_frame = starts; in.cap_contours_per_frame = contours; in.cap_points_per_frame = points;
    Ctx c(in);
    if (!c.c) return;
    aslam_detector_params dp;
    aslam_default_detector_params(&dp);
    dp.minMarkerPerimeterRate = min_rate; dp.maxMarkerPerimeterRate = max_rate;
    OK(aslam_set_detector_params(c, &dp));
    Image bad(rows, cols, 1, 0), good(rows, cols, 1, 0);
    if (kind == 0) { for (int y = 1; y < 31; y++) for (int x = 1; x < 61; x++) if ((x + y) % 2 == 0) bad.set(y, x, 0); }
    else if (kind == 1) { int k = 0; for (int y = 1; y < rows - 4; y += 4) for (int x = 1; x < cols - 4; x += 4) if (k++ < 40) bad.ring(x, y, 3, 3); }
    else {
        int x0 = 2, y0 = 2, x1 = cols - 3, y1 = rows - 3;
        const int step = 3;
        while (x1 - x0 > 2 * step && y1 - y0 > 2 * step) {
            bad.rect(x0, y0, x1 - x0 + 1, 1, 0); bad.rect(x1, y0, 1, y1 - y0 + 1, 0); bad.rect(x0 + step, y1, x1 - x0 - step + 1, 1, 0);
            bad.rect(x0 + step, y0 + step, 1, y1 - y0 - step + 1, 0); bad.rect(x0 + step, y0 + step, x1 - x0 - 2 * step + 1, 1, 0);
            x0 += step; y0 += step; x1 -= step; y1 -= step;
        }
    }
    good.ring(5, 5, 20, 20);
    OK(aslam_stage_frames(c, 0, bad.px.data(), 1, rows, cols, 1, bad.step, bad.px.size()));
    EXPECT(aslam_debug_run_contours(c, 0, 1, 64, -1), ASLAM_E_CAPACITY);
    EXPECT(aslam_debug_run_contours(c, 0, 1, 64, 0), ASLAM_E_CAPACITY);
    OK(aslam_stage_frames(c, 0, good.px.data(), 1, rows, cols, 1, good.step, good.px.size()));
    OK(aslam_debug_run_contours(c, 0, 1, 64, -1));
    OK(aslam_debug_run_contours(c, 0, 1, 32, 0));
}
void capacity_starts() { contour_capacity(256, 1u << 10, 1u << 14, 0, 0.03, 4.0); }
void capacity_contours() { contour_capacity(1u << 13, 32, 1u << 14, 1, 0.03, 4.0); }
void capacity_points() { contour_capacity(1u << 13, 1u << 10, 512, 2, 0.03, 40.0); }

// 129 identified quads: the first 128 are kept, the markers overflow is reported at the sync
void candidates_129() {
    aslam_init in = small_init(24, 8, 1);
    in.max_rows = 240; in.max_cols = 320;
    Ctx c(in);
    if (!c.c) return;
    OK(aslam_set_camera(c, kCamK, kCamD, 5));
    for (int n : {128, 129}) {
        std::vector<int> ids(n), rots(n);
        std::vector<float> cr(8 * (size_t)n);
        for (int k = 0; k < n; k++) {
            ids[k] = 1023 - k; rots[k] = k % 4;
            const float x = 4.0f + 19.0f * (k % 16), y = 4.0f + 19.0f * (k / 16), w = 14.0f;
            const float q[8] = {x, y, x + w, y, x + w, y + w, x, y + w};
            std::memcpy(&cr[8 * (size_t)k], q, sizeof q);
        }
        OK(aslam_debug_inject_candidates(c, 0, n, ids.data(), rots.data(), cr.data()));
        OK(aslam_debug_run_pose(c, 0, 1, nullptr));
        EXPECT(aslam_sync(c), n == 129 ? ASLAM_E_CAPACITY : ASLAM_OK);
        int M = 0; std::vector<int> mi(128); std::vector<float> mc(1024); std::vector<double> rv(384), tv(384);
        OK(aslam_get_slot_detections(c, 0, &M, mi.data(), mc.data(), rv.data(), tv.data()));
        CHECK(M == 128, "%d candidates gave %d markers", n, M);
        CHECK(all_finite(rv) && all_finite(tv), "a pose of the %d-candidate list is not finite", n);
    }
}

// the host-fed stream (tests/test_host_stream_paths.py): a ring of 2 x 2 frames, six frames pushed: the ring wraps once
void stream_wrap() {
    aslam_init in = small_init(24, 16, 4);
    in.max_rows = 240; in.max_cols = 320;
    Ctx c(in);
    if (!c.c) return;
    OK(aslam_set_camera(c, kCamK, kCamD, 5));
    const int mids[4] = {7, 100, 513, 1023};
    double poses[48];
    std::vector<uint8_t> host((size_t)240 * 320);
    OK(aslam_stream_open(c, 240, 320, 1, 2));
    for (int f = 0; f < 6; f++) {
        marker_poses(1.5 + 0.07 * f, poses);
        OK(aslam_synth_render(c, 3, 240, 320, kCamK, 4, mids, poses, 0.27, 200, 2, 10 + f, 1, host.data()));
        if (f % 2) OK(aslam_stream_push(c, host.data(), 320, f ? WL : 0, f ? WR : 0, f ? DT : 0));
        else {
            uint8_t* px = nullptr; size_t step = 0;
            OK(aslam_stream_acquire(c, &px, &step));
            if (!px) return;
            for (int y = 0; y < 240; y++) std::memcpy(px + (size_t)y * step, &host[(size_t)y * 320], 320);
            OK(aslam_stream_commit(c, f ? WL : 0, f ? WR : 0, f ? DT : 0));
        }
    }
    OK(aslam_stream_flush(c));
    check_state(c, 4);
    check_stats(c, 1, 4, 0, 4, 0);                         // the sixth frame: half 0 of the ring again, its second slot
}

void image_and_stream_scenarios() {
    scenario("image/small_gray", image_small_gray);
    scenario("image/small_bgr", image_small_bgr);
    scenario("image/synth_240x320", image_synth);
    scenario("image/capacity_starts", capacity_starts);
    scenario("image/capacity_contours", capacity_contours);
    scenario("image/capacity_points", capacity_points);
    scenario("image/candidates_129", candidates_129);
    scenario("stream/ring_wrapped_once", stream_wrap);
}
void window_to_rig_scenarios() {
    scenario("window/set_20", window_20);
    scenario("window/set_21", window_21);
    scenario("window/set_41", window_41);
    scenario("window/set_42", window_42);
    scenario("window/set_63", window_63);
    scenario("window/handover", window_handover);
    scenario("window/handover_split", window_handover_split);
    scenario("window/gated", window_gated);
    scenario("window/consistent", window_consistent);
    scenario("window/then_augment", window_then_augment);
    scenario("window/pieces", window_pieces);
    scenario("chain/slam_gate", chain_gated);
    scenario("fleet_slam/cap_and_max", fleet_slam);
    scenario("map_edit/ld63", map_edit_ld63);
    scenario("map_edit/large", map_edit_large);
    scenario("merge/two_maps_1024", merge_two_1024);
    scenario("merge/256_maps_40", merge_256_40);
    scenario("merge/dup_and_range", merge_dup_range);
    scenario("reloc/localize", reloc_localize);
    scenario("reloc/fleet", reloc_fleet);
    scenario("reloc/slam", reloc_slam);
    scenario("confirm/128", confirm_128);
    scenario("confirm/1", confirm_1);
    scenario("rig/lists_128_129", rig_lists);
    scenario("rig/slam_step", rig_slam_step);
}

}  // namespace

int main() {
    const auto t0 = std::chrono::steady_clock::now();
    scenario("chain/fast_24_24", chain_fast);
    scenario("chain/mid_64_64", chain_mid);
    scenario("chain/general_128_128", chain_general);
    scenario("chain/fast_ld0", chain_fast_ld0);
    scenario("chain/mid_ld1", chain_mid_ld1);
    scenario("chain/general_ld63", chain_general_ld63);
    scenario("chain/mid_33", chain_mid_33);
    scenario("chain/full_list_128", chain_full_list);
    scenario("augment/fill_to_max", augment_fill);
    scenario("augment/over_by_one", augment_over_by_one);
    scenario("augment/id_edges", augment_id_edges);
    scenario("loc/policy_0", loc_p0);
    scenario("loc/policy_1_umap", loc_p1);
    scenario("loc/policy_2_gate", loc_p2);
    scenario("loc/policy_3", loc_p3);
    scenario("loc/policy_4_consistent", loc_p4);
    scenario("loc/policy_5", loc_p5);
    scenario("loc/policy_6", loc_p6);
    scenario("loc/policy_7", loc_p7);
    scenario("loc/L1", loc_L1);
    scenario("loc/L1_uncertain", loc_L1_uncertain);
    scenario("loc/uncertain_largest", loc_uncertain_largest);
    scenario("fleet/policy_0", fleet_p0);
    scenario("fleet/policy_1_umap", fleet_p1);
    scenario("fleet/policy_2_gate", fleet_p2);
    scenario("fleet/policy_3", fleet_p3);
    scenario("fleet/policy_4_consistent", fleet_p4);
    scenario("fleet/policy_5", fleet_p5);
    scenario("fleet/policy_6", fleet_p6);
    scenario("fleet/policy_7", fleet_p7);
    scenario("fleet/one_robot", fleet_one_robot);
    scenario("fleet/one_robot_uncertain", fleet_one_robot_uncertain);
    window_to_rig_scenarios();
    image_and_stream_scenarios();
    int missing = 0;
    for (int i = 0; i < kSpans; i++) {
        std::printf("span %-24s %lld calls\n", g_names[i] ? g_names[i] : "?", g_calls[i]);
        if (g_calls[i] < 1) missing++;
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("%d scenarios, %d failed, %d of %d spans never ran, %.1f s\n", g_run, g_failed, missing, kSpans, s);
    if (g_failed || missing) return 1;
    std::printf("emu_sanitized_check ok\n");
    return 0;
}
