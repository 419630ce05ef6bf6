// Stand-alone driver of tests/test_lbfgs_device_emu_cpu.py: the device-resident L-BFGS of the smplify path restated on the CPU,
// operation by operation. csrc/rc_lbfgs_dev.h (the algorithm, included as it is) runs here on a backend that keeps one std::vector
// per basis index and shares no addressing with the library. With Real = float every vector operation is the fp32 chain the kernels
// of csrc/rc_smplify.hip compute -- rc_vec_axpy / rc_vec_comb fused (fmaf), rc_vec_pair separate, rc_vec_dots in double in the
// kernel's order (16 elements per thread at stride 256, the xor butterfly of a wave, waves 0..3, blocks in order), the total as
// total_loss of csrc/rc_smplify_api.cpp -- and the closure is rc_syn_closure_* (only + - *, no contraction), so a run of
// rc_lbfgs_device_probe on the GPU has to reproduce every recorded bit (tests/test_gpu_lbfgs_device_exact.py). With Real = double
// and plain dots the same program is anchored to rc::Lbfgs<double> through the library (rc_lbfgs_minimize).
//   g++ -std=c++17 -O1 -ffp-contract=off -Wall -Wextra -Werror -I robustcap_amd/csrc tests/lbfgs_device_emu.cpp -o lbfgs_device_emu
//   lbfgs_device_emu [--real double] [--mutate NAME] [--list-mutations]        one JSON line per case
#include "rc_lbfgs_dev.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>

static void require(bool ok, const char* what) {
    if (!ok) { std::fprintf(stderr, "lbfgs_device_emu: %s\n", what); std::exit(2); }
}

enum Mutation {
    kNone, kGsumFromGmax, kDmaxFromG, kDirectionAfterPoint, kAcceptAfterPoint, kYSwapped, kSFromNewDirection, kEvictNewest,
    kPairOverKeptSlot, kFirstBlockOnly, kShortRowExtended, kLastElementDropped, kTrialIntoBracketSlot, kSYCoefSwapped, kDotsFp32,
    kCombDouble, kImuOnce, kAxpyUnfused, kNumMutations
};
static const char* const kMutationName[kNumMutations] = {
    "none", "gsum_from_gmax", "dmax_from_g", "direction_after_point", "accept_after_point", "y_swapped", "s_from_new_direction",
    "evict_newest", "pair_over_kept_slot", "first_block_only", "short_row_extended", "last_element_dropped",
    "trial_into_bracket_slot", "s_y_coef_swapped", "dots_fp32", "comb_double", "imu_once", "axpy_unfused"};
static Mutation g_mut = kNone;

// every fp32 intermediate is zero or a normal number: no result depends on how subnormals are handled
template <class R> static R N(R v) {
    if (std::is_same<R, float>::value && g_mut == kNone) require(v == 0 || std::isnormal(v), "an fp32 intermediate is neither zero nor normal");
    return v;
}
// a b + c as rc_vec_axpy / rc_vec_comb form it: fp32 fused (one rounding); Real = double is the plain anchor, two roundings as in rc_lbfgs.h
static float fused(float a, float b, float c) { return N(std::fma(a, b, c)); }
static double fused(double a, double b, double c) { return a * b + c; }

// ---------------------------------------------------------------------------------------------------------------- the closure
// rc_syn_closure_* of csrc/rc_smplify.hip, the operations in the kernel's order; in double the same formulas (the anchor)
template <class R>
struct Objective {
    int T = 0;
    std::vector<R> a, b;
    R imu_w = 0;                                                    // 0.5 / T, rounded once
    R eval(const std::vector<R>& x, std::vector<R>& g) const {
        const long long n = 75LL * T;
        for (long long i = 0; i < n; ++i) {                        // syn_grad_elem
            const R xi = x[i], u = N(xi - b[i]);
            const R uu = N(u * u);
            R au = N(a[i] * u);
            au = N(au + au);
            R gi = N(au + N(uu * u));
            if (i + 1 < n) { const R w = N(x[i + 1] - N(xi * xi)); const R p = N(xi * w); gi = N(gi - N(R(8) * p)); }
            if (i > 0) { const R xm = x[i - 1]; const R wm = N(xi - N(xm * xm)); gi = N(gi + N(R(4) * wm)); }
            if (i % 75 == 0) gi = N(gi + u);
            g[i] = gi;
        }
        std::vector<R> terms((size_t)3 * T);
        for (int t = 0; t < T; ++t) {                              // syn_terms_frame
            R f = 0, sm = 0;
            for (int e = 0; e < 75; ++e) {
                const long long i = 75LL * t + e;
                const R xi = x[i], u = N(xi - b[i]);
                const R uu = N(u * u);
                const R q = N(a[i] * uu);
                R r = N(uu * uu);
                r = N(R(0.25) * r);
                f = N(f + N(q + r));
                if (i + 1 < n) { const R w = N(x[i + 1] - N(xi * xi)); const R ww = N(w * w); sm = N(sm + N(ww + ww)); }
            }
            const R u0 = N(x[75LL * t] - b[75LL * t]);
            terms[t] = f; terms[2 * T + t] = sm; terms[T + t] = N(imu_w * N(u0 * u0));
        }
        double F = 0.0, I = 0.0, S = 0.0;                           // total_loss: the IMU term counts T times
        for (int t = 0; t < T; ++t) { F += terms[t]; I += terms[T + t]; S += terms[2 * T + t]; }
        return R(F + (g_mut == kImuOnce ? 1.0 : (double)T) * I + S);
    }
};

// ------------------------------------------------------------------------------------------------- rc_vec_dots, the kernel's order
// op 0: sum a b, 1: max |a|, 2: sum |a|
static double stale_partial = 0.0;                                   // (kShortRowExtended: what another row left behind)
static double dots_kernel(int op, const std::vector<float>& a, const std::vector<float>& b, int nb_round) {
    long long n = (long long)a.size();
    const int nb = (int)((n + 4095) / 4096);
    if (g_mut == kLastElementDropped) --n;
    std::vector<double> part((size_t)nb);
    for (int blk = 0; blk < nb; ++blk) {
        double acc[256];
        float acc32[256];
        for (int tid = 0; tid < 256; ++tid) {
            double s = 0.0; float s32 = 0.0f;
            for (int q = 0; q < 16; ++q) {
                const long long i = (long long)blk * 4096 + q * 256 + tid;
                if (i >= n) continue;
                const double v = a[(size_t)i];
                if (op == 0) { s = std::fma(v, (double)b[(size_t)i], s); s32 += a[(size_t)i] * b[(size_t)i]; }
                else if (op == 1) { s = std::fmax(s, std::fabs(v)); s32 = std::fmax(s32, std::fabs(a[(size_t)i])); }
                else { s += std::fabs(v); s32 += std::fabs(a[(size_t)i]); }
            }
            acc[tid] = s; acc32[tid] = s32;
        }
        if (g_mut == kDotsFp32) for (int tid = 0; tid < 256; ++tid) acc[tid] = acc32[tid];
        double red[4];
        for (int w = 0; w < 4; ++w) {                                // the xor butterfly: every lane of every stage, lane 0 read at the end
            double v[64], nv[64];
            for (int l = 0; l < 64; ++l) v[l] = acc[w * 64 + l];
            for (int off = 32; off > 0; off >>= 1) {
                for (int l = 0; l < 64; ++l) {
                    nv[l] = op == 1 ? std::fmax(v[l], v[l ^ off]) : v[l] + v[l ^ off];
                    if (g_mut == kDotsFp32) nv[l] = (float)nv[l];
                }
                std::memcpy(v, nv, sizeof(v));
            }
            red[w] = v[0];
        }
        double r = red[0];
        for (int w = 1; w < 4; ++w) { r = op == 1 ? std::fmax(r, red[w]) : r + red[w]; if (g_mut == kDotsFp32) r = (float)r; }
        part[(size_t)blk] = r;
    }
    double r = part[0];                                              // part_sum: blocks in order
    if (g_mut != kFirstBlockOnly) for (int k = 1; k < nb; ++k) r = op == 1 ? std::fmax(r, part[(size_t)k]) : r + part[(size_t)k];
    if (g_mut == kShortRowExtended) {
        for (int k = nb; k < nb_round; ++k) r = op == 1 ? std::fmax(r, stale_partial) : r + stale_partial;
        stale_partial = part[(size_t)nb - 1];
    }
    return r;
}
static double dots_kernel(int op, const std::vector<double>& a, const std::vector<double>& b, int) {   // Real = double: plain
    double r = 0.0;
    for (size_t i = 0; i < a.size(); ++i) r = op == 0 ? r + a[i] * b[i] : (op == 1 ? std::fmax(r, std::fabs(a[i])) : r + std::fabs(a[i]));
    return r;
}

// -------------------------------------------------------------------------------------------------------------------- the backend
template <class R>
struct Backend {
    using Dev = rc::LbfgsDev<R>;
    const Objective<R>& obj;
    const int P, nb_round;                                           // physical pair slots; block count of the longest row of a batch
    std::vector<R> x, xt, d;
    std::vector<std::vector<R>> basis;                               // [2 P + kSlots]: s, y, gradient slots
    // what the test's census reads
    std::vector<std::vector<double>> steps;                          // per iteration, the t of every evaluation
    std::vector<int> n_terms, jobs, pair_slots;                      // terms of every direction; inner products of every request; slot of every candidate pair
    int n_vec_ops = 0, max_slot = 0;                                 // vector operations launched; highest gradient slot written
    // mutations that move an operation
    std::vector<typename Dev::Term> late_terms;
    bool have_late_x = false; std::vector<R> late_x;
    int last_c = -1; R last_t = 0;
    int base_slot = 0, alias[6] = {0, 1, 2, 3, 4, 5};

    Backend(const Objective<R>& o, const std::vector<R>& x0, int pairs, int nbr)
        : obj(o), P(pairs), nb_round(nbr), x(x0), xt(x0.size()), d(x0.size(), R(0)), basis((size_t)2 * pairs + Dev::kSlots, std::vector<R>(x0.size(), R(0))) {}
    std::vector<R>& vec(int i) {
        require(i >= 0 && i < 2 * P + Dev::kSlots, "basis index out of range");
        return basis[(size_t)i];
    }
    void form_direction(const typename Dev::Term* terms, int n) {   // rc_vec_comb: acc = fmaf(c_k, v_k[i], acc) from acc = 0
        for (size_t i = 0; i < d.size(); ++i) {
            R acc = 0; double wide = 0.0;
            for (int q = 0; q < n; ++q) {
                int v = terms[q].vec;
                if (g_mut == kSYCoefSwapped && v < 2 * P) v = v < P ? v + P : v - P;
                acc = fused(terms[q].coef, vec(v)[i], acc);
                wide += (double)terms[q].coef * (double)vec(v)[i];
            }
            d[i] = g_mut == kCombDouble ? R(wide) : acc;
        }
        if (g_mut == kSFromNewDirection && last_c >= 0) for (size_t i = 0; i < d.size(); ++i) vec(last_c)[i] = d[i] * last_t;
    }
    void axpy(const std::vector<R>& from, R t, std::vector<R>& to) {   // rc_vec_axpy: fmaf(t, d[i], x[i])
        for (size_t i = 0; i < from.size(); ++i) to[i] = g_mut == kAxpyUnfused ? R(from[i] + R(t * d[i])) : fused(t, d[i], from[i]);
    }
    bool eval(R t, int k, typename Dev::Eval& e) {
        require(k >= 0 && k < Dev::kSlots, "gradient slot out of range");
        if (steps.empty()) steps.emplace_back();
        steps.back().push_back((double)t);
        jobs.push_back(5);
        max_slot = std::max(max_slot, k);
        if (g_mut == kTrialIntoBracketSlot) {                       // the fourth live slot lands on the bracket end at x
            alias[k] = k >= 3 ? alias[base_slot] : k;
            k = alias[k];
        }
        if (!late_terms.empty() && g_mut != kDirectionAfterPoint) { form_direction(late_terms.data(), (int)late_terms.size()); late_terms.clear(); }
        if (t != 0) { axpy(x, t, xt); ++n_vec_ops; } else xt = x;
        if (!late_terms.empty()) { form_direction(late_terms.data(), (int)late_terms.size()); late_terms.clear(); }
        if (have_late_x) { x = late_x; have_late_x = false; }
        std::vector<R>& g = vec(2 * P + k);
        e.f = obj.eval(xt, g);
        e.gtd = R(dots_kernel(0, g, d, nb_round));
        e.gmax = R(dots_kernel(1, g, g, nb_round));
        e.gsum = g_mut == kGsumFromGmax ? e.gmax : R(dots_kernel(2, g, g, nb_round));
        e.dmax = R(dots_kernel(1, g_mut == kDmaxFromG ? g : d, d, nb_round));
        e.gg = R(dots_kernel(0, g, g, nb_round));
        return true;
    }
    void direction(const typename Dev::Term* terms, int n) {
        steps.emplace_back(); n_terms.push_back(n); ++n_vec_ops;
        late_terms.assign(terms, terms + n);                         // formed in front of the next evaluation
    }
    void accept(R t) {
        ++n_vec_ops;
        if (g_mut == kAcceptAfterPoint) { late_x = x; axpy(x, t, late_x); have_late_x = true; return; }
        axpy(x, t, x);
    }
    bool pair(int c, int g_new, int g_old, R t, const typename Dev::Want* want, int n_want, double* out) {
        require(c >= 0 && c < P, "pair slot out of range");
        require(g_new >= 0 && g_new < Dev::kSlots && g_old >= 0 && g_old < Dev::kSlots, "gradient slot out of range");
        ++n_vec_ops;
        jobs.push_back(n_want); pair_slots.push_back(c);
        if (g_mut == kTrialIntoBracketSlot) { base_slot = g_new; g_new = alias[g_new]; g_old = alias[g_old]; }
        int to = c;
        if (g_mut == kEvictNewest && last_c >= 0 && n_want >= 6 * P) to = last_c;      // history full: over the newest pair
        if (g_mut == kPairOverKeptSlot && n_want > 6) to = (c + 1) % P;
        const std::vector<R> &gn = vec(2 * P + g_new), &go = vec(2 * P + g_old);
        std::vector<R> &s = vec(to), &y = vec(P + to);
        for (size_t i = 0; i < x.size(); ++i) {                      // rc_vec_pair
            y[i] = g_mut == kYSwapped ? N(go[i] - gn[i]) : N(gn[i] - go[i]);
            s[i] = N(d[i] * t);
        }
        last_c = c; last_t = t;
        for (int q = 0; q < n_want; ++q) out[q] = dots_kernel(0, vec(want[q].a), vec(want[q].b), nb_round);
        return true;
    }
    bool flush() {
        if (have_late_x) { x = late_x; have_late_x = false; }
        return true;
    }
};

// ------------------------------------------------------------------------------------------------------------------------ the cases
// inputs from a seed, every value exact in fp32: a in [0.5, 2.5), b in [-1, 1), x0 in [-0.5, 0.5) scaled by x_scale
static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
struct Case { const char* name; int T; uint32_t seed; double lr; int max_iter, history; double x_scale; int nb_round; };
// history: RC_LBFGS_HISTORY of the run (0: unset); nb_round: block count of the longest row of the batch the case stands in
static const Case kCases[] = {
    {"prod_T1", 1, 9, 1e-3, 20, 0, 1.0, 2},       {"prod_T54", 54, 8, 1e-3, 20, 0, 1.0, 2},       {"prod_T55", 55, 80, 1e-3, 20, 0, 1.0, 2},
    {"hist2_T1", 1, 9, 1.0, 12, 2, 1.0, 2},       {"hist2_T54", 54, 8, 1.0, 12, 2, 1.0, 2},       {"hist2_T55", 55, 80, 1.0, 12, 2, 1.0, 2},
    {"hist4_T1", 1, 9, 1.0, 60, 4, 1.0, 2},       {"hist4_T54", 54, 8, 1.0, 60, 4, 1.0, 2},       {"hist4_T55", 55, 80, 1.0, 60, 4, 1.0, 2},
    {"prod_zero", 1, 0, 1e-3, 20, 0, 0.0, 2},     {"hist2_zero", 1, 0, 1.0, 12, 2, 0.0, 2},        {"hist4_zero", 1, 0, 1.0, 60, 4, 0.0, 2},
    {"grid_0", 1, 100, 1.0, 25, 0, 1.0, 1},      {"grid_1", 1, 101, 1.0, 25, 0, 1.0, 1},         {"grid_2", 1, 102, 1.0, 25, 0, 1.0, 1},
    {"grid_3", 1, 103, 1.0, 25, 0, 1.0, 1},      {"grid_4", 1, 104, 1.0, 25, 0, 1.0, 1},         {"grid_5", 1, 105, 1.0, 25, 0, 1.0, 1},
    {"grid_6", 1, 106, 1.0, 25, 0, 1.0, 1},      {"grid_7", 1, 107, 1.0, 25, 0, 1.0, 1}};

template <class R> static void print_bits(const char* key, const std::vector<R>& v) {
    std::printf("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); ++i) {
        if (std::is_same<R, float>::value) { const float f = (float)v[i]; uint32_t u; std::memcpy(&u, &f, 4); std::printf("%s%u", i ? ", " : "", u); }
        else std::printf("%s%.17g", i ? ", " : "", (double)v[i]);
    }
    std::printf("]");
}

template <class R> static void run(const Case& c) {
    Objective<R> o;
    o.T = c.T;
    const int n = 75 * c.T;
    o.a.resize((size_t)n); o.b.resize((size_t)n);
    o.imu_w = std::is_same<R, float>::value ? R(0.5f / (float)c.T) : R(0.5 / c.T);
    std::vector<R> x0((size_t)n);
    uint32_t s = c.seed;
    for (int i = 0; i < n; ++i) {
        const float av = 0.5f + (float)(lcg(s) % 1024u) / 1024.0f * 2.0f, bv = (float)((int)(lcg(s) % 2048u) - 1024) / 1024.0f;
        const float xv = (float)((int)(lcg(s) % 2048u) - 1024) / 2048.0f;
        o.a[(size_t)i] = av; o.b[(size_t)i] = c.x_scale == 0.0 ? 0.0f : bv; x0[(size_t)i] = (float)c.x_scale * xv;
    }
    // lbfgs_options of csrc/rc_smplify_api.cpp
    typename rc::LbfgsDev<R>::Options op;
    const int hist_env = c.history > 0 ? c.history : 100;
    op.lr = R((float)c.lr); op.max_iter = c.max_iter; op.max_eval = c.max_iter * 5 / 4;
    op.history_size = std::max(1, std::min(std::min(c.max_iter, 100), hist_env));
    Backend<R> be(o, x0, op.history_size + 1, c.nb_round);
    typename rc::LbfgsDev<R>::Result r;
    require(rc::LbfgsDev<R>::minimize(be, op, r), "the backend does not fail");
    require((int)r.losses.size() == r.n_eval, "one loss per evaluation");
    std::printf("{\"name\": \"%s\", \"T\": %d, \"seed\": %u, \"lr\": %.17g, \"max_iter\": %d, \"history_env\": %d, \"x_scale\": %.17g, \"history\": %d, "
                "\"max_eval\": %d, \"n_iter\": %d, \"n_eval\": %d, \"n_vec_ops\": %d, \"max_slot\": %d, ",
                c.name, c.T, c.seed, c.lr, c.max_iter, c.history, c.x_scale, op.history_size, op.max_eval, r.n_iter, r.n_eval, be.n_vec_ops, be.max_slot);
    print_bits("losses", r.losses);
    std::printf(", ");
    print_bits("x", be.x);
    std::printf(", \"steps\": [");
    for (size_t i = 0; i < be.steps.size(); ++i) {
        std::printf("%s[", i ? ", " : "");
        for (size_t k = 0; k < be.steps[i].size(); ++k) {
            if (std::isfinite(be.steps[i][k])) std::printf("%s%.9g", k ? ", " : "", be.steps[i][k]);
            else std::printf("%snull", k ? ", " : "");              // (a mutation's run may leave the numbers)
        }
        std::printf("]");
    }
    std::printf("], \"n_terms\": [");
    for (size_t i = 0; i < be.n_terms.size(); ++i) std::printf("%s%d", i ? ", " : "", be.n_terms[i]);
    std::printf("], \"jobs\": [");
    for (size_t i = 0; i < be.jobs.size(); ++i) std::printf("%s%d", i ? ", " : "", be.jobs[i]);
    std::printf("], \"pair_slots\": [");
    for (size_t i = 0; i < be.pair_slots.size(); ++i) std::printf("%s%d", i ? ", " : "", be.pair_slots[i]);
    std::printf("]}\n");
}

int main(int argc, char** argv) {
    bool use_double = false, have_extra = false;
    Case extra{};
    for (int i = 1; i < argc; ++i) {
        const std::string arg = argv[i];
        if (arg == "--list-mutations") { for (int m = 1; m < kNumMutations; ++m) std::printf("%s\n", kMutationName[m]); return 0; }
        else if (arg == "--real" && i + 1 < argc) use_double = std::string(argv[++i]) == "double";
        else if (arg == "--mutate" && i + 1 < argc) {
            const std::string name = argv[++i];
            g_mut = kNumMutations;
            for (int m = 0; m < kNumMutations; ++m) if (name == kMutationName[m]) g_mut = (Mutation)m;
            require(g_mut != kNumMutations, "unknown mutation");
        } else if (arg == "--case" && i + 7 < argc) {                  // T seed lr max_iter history x_scale nb_round: one case of the caller's
            extra = Case{"custom", std::atoi(argv[i + 1]), (uint32_t)std::atoll(argv[i + 2]), std::atof(argv[i + 3]), std::atoi(argv[i + 4]),
                         std::atoi(argv[i + 5]), std::atof(argv[i + 6]), std::atoi(argv[i + 7])};
            have_extra = true; i += 7;
        } else require(false, "usage: lbfgs_device_emu [--real double] [--mutate NAME] [--list-mutations] [--case T seed lr max_iter history x_scale nb_round]");
    }
    require(!(use_double && g_mut != kNone), "mutations belong to the float backend");
    if (have_extra) { if (use_double) run<double>(extra); else run<float>(extra); return 0; }
    for (const Case& c : kCases) { stale_partial = 0.0; if (use_double) run<double>(c); else run<float>(c); }
    return 0;
}
