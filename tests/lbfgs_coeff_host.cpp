// Stand-alone driver of tests/test_lbfgs_coeff_cpu.py: the coefficient-space L-BFGS of csrc/rc_lbfgs_dev.h, in double over
// std::vector, next to rc::Lbfgs<double> (csrc/rc_lbfgs.h, which tests/test_lbfgs_host.py pins to torch.optim.LBFGS) on the same
// objectives and starting points. Prints one JSON line per case with both records. The backend also checks what the algorithm
// hands it: every index in range, and a candidate pair never written over one of the pairs the last direction was built from.
//   g++ -std=c++17 -I robustcap_amd/csrc tests/lbfgs_coeff_host.cpp -o lbfgs_coeff_host
#include "rc_lbfgs_dev.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>

using Dev = rc::LbfgsDev<double>;
using L = rc::Lbfgs<double>;

static void require(bool ok, const char* what) {
    if (!ok) { std::fprintf(stderr, "lbfgs_coeff_host: %s\n", what); std::exit(2); }
}

static double rosenbrock(const L::Vec& x, L::Vec& g) {
    double f = 0.0;
    std::fill(g.begin(), g.end(), 0.0);
    for (size_t i = 0; i + 1 < x.size(); ++i) {
        const double a = x[i + 1] - x[i] * x[i], b = 1.0 - x[i];
        f += 100.0 * a * a + b * b;
        g[i] += -400.0 * x[i] * a - 2.0 * b;
        g[i + 1] += 200.0 * a;
    }
    return f;
}
// non-smooth (|.|) + exponential terms, like the smoothness and angle-prior terms of the fitting loss
static double kinked(const L::Vec& x, L::Vec& g) {
    double f = 0.0;
    for (size_t i = 0; i < x.size(); ++i) {
        const double v = x[i], u = v - 0.3;
        f += std::exp(0.3 * v) + 0.1 * v * v * v * v + std::fabs(u) + std::sin(3.0 * v);
        g[i] = 0.3 * std::exp(0.3 * v) + 0.4 * v * v * v + (u > 0 ? 1.0 : (u < 0 ? -1.0 : 0.0)) + 3.0 * std::cos(3.0 * v);
    }
    return f;
}

struct VectorBackend {
    L::Objective fn;
    int P;
    L::Vec x, xt, d;
    std::vector<L::Vec> basis;                   // [2 P + kSlots]: s, y, gradient slots
    std::set<int> kept;                          // pairs the last direction was built from

    VectorBackend(L::Objective f, const L::Vec& x0, int pairs)
        : fn(std::move(f)), P(pairs), x(x0), xt(x0.size()), d(x0.size(), 0.0), basis((size_t)2 * pairs + Dev::kSlots, L::Vec(x0.size(), 0.0)) {}
    L::Vec& vec(int i) {
        require(i >= 0 && i < 2 * P + Dev::kSlots, "basis index out of range");
        return basis[(size_t)i];
    }
    bool eval(double t, int k, Dev::Eval& e) {
        require(k >= 0 && k < Dev::kSlots, "gradient slot out of range");
        L::Vec& g = vec(2 * P + k);
        for (size_t i = 0; i < x.size(); ++i) xt[i] = t != 0.0 ? x[i] + t * d[i] : x[i];
        e.f = fn(xt, g);
        e.gtd = L::dot(g, d); e.gmax = L::abs_max(g); e.gsum = L::abs_sum(g); e.dmax = L::abs_max(d); e.gg = L::dot(g, g);
        return true;
    }
    void direction(const Dev::Term* terms, int n) {
        kept.clear();
        std::fill(d.begin(), d.end(), 0.0);
        for (int q = 0; q < n; ++q) {
            const L::Vec& v = vec(terms[q].vec);
            if (terms[q].vec < P) kept.insert(terms[q].vec);
            for (size_t i = 0; i < d.size(); ++i) d[i] += terms[q].coef * v[i];
        }
    }
    void accept(double t) { for (size_t i = 0; i < x.size(); ++i) x[i] += t * d[i]; }
    bool pair(int c, int g_new, int g_old, double t, const Dev::Want* want, int n_want, double* out) {
        require(c >= 0 && c < P, "pair slot out of range");
        require(g_new >= 0 && g_new < Dev::kSlots && g_old >= 0 && g_old < Dev::kSlots, "gradient slot out of range");
        require(kept.count(c) == 0, "candidate pair written over a pair that is kept");
        const L::Vec &gn = vec(2 * P + g_new), &go = vec(2 * P + g_old);
        L::Vec &s = vec(c), &y = vec(P + c);
        for (size_t i = 0; i < x.size(); ++i) { y[i] = gn[i] - go[i]; s[i] = d[i] * t; }
        for (int q = 0; q < n_want; ++q) out[q] = L::dot(vec(want[q].a), vec(want[q].b));
        return true;
    }
    bool flush() { return true; }
};

static void print_record(const char* key, const L::Result& r, const L::Vec& x) {
    std::printf("\"%s\": {\"n_iter\": %d, \"n_eval\": %d, \"losses\": [", key, r.n_iter, r.n_eval);
    for (size_t i = 0; i < r.losses.size(); ++i) std::printf("%s%.17g", i ? ", " : "", r.losses[i]);
    std::printf("], \"x\": [");
    for (size_t i = 0; i < x.size(); ++i) std::printf("%s%.17g", i ? ", " : "", x[i]);
    std::printf("]}");
}

static L::Vec linspace(double a, double b, int n) {
    L::Vec v((size_t)n);
    for (int i = 0; i < n; ++i) v[(size_t)i] = a + (b - a) * i / (n - 1);
    return v;
}

int main() {
    struct Case { const char* name; L::Objective fn; L::Vec x0; double lr; int max_iter, history; };
    const Case cases[] = {{"rosen_lr1", rosenbrock, linspace(-1.2, 1.0, 10), 1.0, 20, 100},
                          {"rosen_lr1e-3", rosenbrock, linspace(-1.2, 1.0, 10), 1e-3, 20, 100},
                          {"rosen_short_history", rosenbrock, linspace(-1.2, 1.0, 10), 1.0, 60, 4},
                          {"rosen_history1", rosenbrock, linspace(-1.2, 1.0, 10), 1.0, 60, 1},
                          {"kinked", kinked, linspace(-2, 2, 37), 0.5, 40, 100},
                          {"kinked_lr1e-3", kinked, linspace(-2, 2, 37), 1e-3, 20, 100},
                          {"at_optimum", rosenbrock, L::Vec(6, 1.0), 1.0, 20, 100}};
    for (const Case& c : cases) {
        L::Options o;                                       // tolerances: the defaults, as in test_lbfgs_host.py
        o.lr = c.lr; o.max_iter = c.max_iter; o.max_eval = c.max_iter * 5 / 4; o.history_size = c.history;
        L::Vec xh = c.x0;
        const L::Result host = L::minimize(c.fn, xh, o);
        VectorBackend be(c.fn, c.x0, c.history + 1);
        L::Result dev;
        require(Dev::minimize(be, o, dev), "the backend does not fail");
        std::printf("{\"name\": \"%s\", ", c.name);
        print_record("coeff", dev, be.x);
        std::printf(", ");
        print_record("host", host, xh);
        std::printf("}\n");
    }
    return 0;
}
