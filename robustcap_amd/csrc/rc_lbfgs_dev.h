// L-BFGS with a strong-Wolfe line search over vectors that stay wherever a backend keeps them (the device), host side.
//
// The optimiser of rc_lbfgs.h (torch.optim.LBFGS(max_iter, strong_wolfe)), restated so that no vector is touched here: it consumes
// scalars -- per closure evaluation f, g.d, |g|_inf, |g|_1, |d|_inf and g.g, per iteration the inner products of the new curvature
// pair and of the gradient with the pairs kept -- and emits coefficients: the two-loop recursion runs in COEFFICIENT space, the
// direction is d = sum_j a_j s_j + b_j y_j + c g with its (2m + 1) coefficients computed in float64, and the backend forms d.
// Vectors are named by BASIS INDEX, never by address:
//     j in [0, P)  s_j          P + j  y_j          2 P + k  gradient slot k (k < kSlots)
// with P = history_size + 1 physical pair slots (see `spare` below). A backend turns indices into addresses and provides
//     bool eval(Real t, int k, Eval& e)        closure at x + t d into gradient slot k (t == 0: at x itself; the products with d
//                                              are then meaningless) and the six scalars of Eval
//     void direction(const Term* terms, int n) d = sum terms[i].coef * vec(terms[i].vec), formed before the next evaluation
//     void accept(Real t)                      x += t d, before anything that next reads x
//     bool pair(int c, int g_new, int g_old, Real t, const Want* want, int n_want, double* out)
//                                              y_c = g(slot g_new) - g(slot g_old), s_c = t d; out[i] = vec(want[i].a) . vec(want[i].b)
//     bool flush()                             whatever is still pending at the end
// (bool: false = the backend failed, minimize returns false at once). rc_smplify_api.cpp holds the two backends of the library;
// tests/lbfgs_coeff_host.cpp runs the algorithm in double over std::vector against rc::Lbfgs<double>; tests/lbfgs_device_emu.cpp runs it in
// float on a backend that restates the library's vector kernels exactly, which the device has to reproduce bit for bit (rc_lbfgs_device_probe).
#pragma once
#include "rc_lbfgs.h"

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <vector>

namespace rc {

template <class Real>
struct LbfgsDev {
    using Host = Lbfgs<Real>;
    using Options = typename Host::Options;
    using Result = typename Host::Result;
    static constexpr int kSlots = 6;      // gradient slots: the one at x, two bracket points, the trial point (and two to spare)
    struct Eval { Real f, gtd, gmax, gsum, dmax, gg; };
    struct Term { int vec; Real coef; };
    struct Want { int a, b; };

    // one optimizer.step(closure) of a fresh torch.optim.LBFGS on the backend's x; false = the backend failed
    template <class Backend>
    static bool minimize(Backend& be, const Options& o, Result& res) {
        // History: the last M curvature pairs (torch: old_dirs.pop(0) when full). M + 1 physical slots: the candidate pair of an
        // iteration goes to the spare one, so that rejecting it (y.s <= 1e-10) leaves the oldest pair alone.
        const int M = std::max(o.history_size, 1), P = M + 1;
        Real slot_gmax[kSlots] = {};                                       // |g|_inf of the last evaluation into each gradient slot
        auto eval = [&](Real t, int k, Eval& e) {
            if (!be.eval(t, k, e)) return false;
            slot_gmax[k] = e.gmax; res.losses.push_back(e.f);
            return true;
        };
        int base = 0;                                                       // slot of the gradient at x
        Eval e0;
        if (!eval(0, base, e0)) return false;
        Real loss = e0.f;
        res.first_loss = res.loss = loss;
        int evals = res.n_eval = 1;
        if (e0.gmax <= o.tolerance_grad) return true;

        // inner products among the basis {s_0.., y_0.., g} by PHYSICAL slot: index j -> s_j, P + j -> y_j, IG -> the gradient at x
        const int IG = 2 * P, NB = IG + 1;
        std::vector<double> G((size_t)NB * NB, 0.0), ro(P, 0.0), al(P, 0.0), delta(NB, 0.0), got;
        auto Gat = [&](int a, int b) -> double& { return G[(size_t)a * NB + b]; };
        std::vector<int> order;                                             // physical slots of the pairs kept, oldest first
        std::vector<Want> want; std::vector<Term> terms;                    // requests of the iteration
        int spare = 0;                                                      // physical slot of the next candidate
        double H_diag = 1.0;
        Real t = 0, prev_loss = loss, gtd = 0, d_max = 0;
        int prev_base = base, n_iter = 0;
        while (n_iter < o.max_iter) {
            ++n_iter;
            terms.clear();
            if (n_iter == 1) {
                terms.push_back({IG + base, Real(-1)});                     // d = -g
                gtd = -e0.gg;                                               // g.d of d = -g
            } else {
                // candidate pair (slot `spare`): y = g - prev_g, s = t d; its inner products with the pairs kept (and itself),
                // those of the gradient with all of them
                const int c = spare;
                std::vector<int> with_c(order); with_c.push_back(c);
                want.clear();
                for (int j : with_c) { want.push_back({c, j}); want.push_back({c, P + j}); want.push_back({P + c, P + j}); }
                for (int j : order) want.push_back({P + c, j});
                const int g = IG + base;                                     // (to the backend: the slot of g)
                for (int j : with_c) { want.push_back({g, j}); want.push_back({g, P + j}); }
                want.push_back({g, g});
                got.resize(want.size());
                if (!be.pair(c, base, prev_base, t, want.data(), (int)want.size(), got.data())) return false;
                for (size_t q = 0; q < want.size(); ++q) { const int a = std::min(want[q].a, IG), b = std::min(want[q].b, IG); Gat(a, b) = Gat(b, a) = got[q]; }
                const double ys = Gat(c, P + c);
                if (Real(ys) > Real(1e-10)) {                                 // keep the pair (torch: ys > 1e-10)
                    H_diag = ys / Gat(P + c, P + c); ro[c] = 1.0 / ys;
                    // history full: the oldest pair goes (old_dirs.pop(0)), its slot takes the next candidate; until then slots go in order
                    if ((int)order.size() == M) { spare = order.front(); order.erase(order.begin()); order.push_back(c); }
                    else { order.push_back(c); spare = (int)order.size(); }
                }
                const int m = (int)order.size();
                // two-loop recursion on coefficients: q = sum_k delta[k] basis[k], starting from q = -g
                std::fill(delta.begin(), delta.end(), 0.0);
                delta[IG] = -1.0;
                auto dot_q = [&](int idx) {
                    double r = delta[IG] * Gat(IG, idx);
                    for (int j : order) r += delta[j] * Gat(j, idx) + delta[P + j] * Gat(P + j, idx);
                    return r;
                };
                for (int i = m - 1; i >= 0; --i) { const int j = order[i]; al[j] = dot_q(j) * ro[j]; delta[P + j] -= al[j]; }
                for (double& v : delta) v *= H_diag;
                for (int i = 0; i < m; ++i) { const int j = order[i]; const double be_ = dot_q(P + j) * ro[j]; delta[j] += al[j] - be_; }
                for (int j : order) { terms.push_back({j, Real(delta[j])}); terms.push_back({P + j, Real(delta[P + j])}); }
                terms.push_back({IG + base, Real(delta[IG])});
                gtd = Real(dot_q(IG));
            }
            be.direction(terms.data(), (int)terms.size());
            prev_base = base;
            prev_loss = loss;
            t = n_iter == 1 ? std::min(Real(1), Real(1) / e0.gsum) * o.lr : o.lr;
            if (gtd > -o.tolerance_change) break;

            // ---- strong-Wolfe line search (rc_lbfgs.h: strong_wolfe) on gradient slots ----------------------------------------
            struct Pt { Real t, f, gtd; int k; };
            const int max_ls = o.max_eval - evals;
            auto free_slot = [&](std::initializer_list<int> live) {
                for (int k = 0; k < kSlots; ++k) { bool used = false; for (int v : live) used = used || v == k; if (!used) return k; }
                return -1;
            };
            const Real c1 = Real(1e-4), c2 = Real(0.9);
            Pt cur{t, 0, 0, free_slot({base})};
            Eval ev;
            if (!eval(cur.t, cur.k, ev)) return false;
            int ls_evals = 1;
            cur.f = ev.f; cur.gtd = ev.gtd; d_max = ev.dmax;
            Pt prev{0, loss, gtd, base};
            Pt br[2] = {prev, prev};
            int n_br = 0, ls_iter = 0;
            bool done = false;
            while (ls_iter < max_ls) {
                if (cur.f > (loss + c1 * cur.t * gtd) || (ls_iter > 1 && cur.f >= prev.f)) { br[0] = prev; br[1] = cur; n_br = 2; break; }
                if (std::fabs(cur.gtd) <= -c2 * gtd) { br[0] = cur; n_br = 1; done = true; break; }
                if (cur.gtd >= 0) { br[0] = prev; br[1] = cur; n_br = 2; break; }
                const Real min_step = cur.t + Real(0.01) * (cur.t - prev.t), max_step = cur.t * 10;
                const Real tn = Host::cubic(prev.t, prev.f, prev.gtd, cur.t, cur.f, cur.gtd, true, min_step, max_step);
                prev = cur;
                cur.t = tn;
                cur.k = free_slot({base, prev.k});
                if (!eval(tn, cur.k, ev)) return false;
                cur.f = ev.f; cur.gtd = ev.gtd;
                ++ls_evals;
                ++ls_iter;
            }
            if (ls_iter == max_ls) { br[0] = Pt{0, loss, gtd, base}; br[1] = cur; n_br = 2; }
            bool insuf = false;
            int lo = 0, hi = 1;
            if (n_br == 2 && !(br[0].f <= br[1].f)) { lo = 1; hi = 0; }
            while (!done && ls_iter < max_ls) {
                if (std::fabs(br[1].t - br[0].t) * d_max < o.tolerance_change) break;
                Real tn = Host::cubic(br[0].t, br[0].f, br[0].gtd, br[1].t, br[1].f, br[1].gtd, false, 0, 0);
                const Real bmax = std::max(br[0].t, br[1].t), bmin = std::min(br[0].t, br[1].t);
                const Real eps = Real(0.1) * (bmax - bmin);
                if (std::min(bmax - tn, tn - bmin) < eps) {
                    if (insuf || tn >= bmax || tn <= bmin) {
                        tn = (std::fabs(tn - bmax) < std::fabs(tn - bmin)) ? bmax - eps : bmin + eps;
                        insuf = false;
                    } else insuf = true;
                } else insuf = false;
                cur.t = tn;
                cur.k = free_slot({base, br[0].k, br[1].k});
                if (!eval(tn, cur.k, ev)) return false;
                cur.f = ev.f; cur.gtd = ev.gtd;
                ++ls_evals;
                ++ls_iter;
                if (cur.f > (loss + c1 * tn * gtd) || cur.f >= br[lo].f) {
                    br[hi] = cur;
                    if (br[0].f <= br[1].f) { lo = 0; hi = 1; } else { lo = 1; hi = 0; }
                } else {
                    if (std::fabs(cur.gtd) <= -c2 * gtd) done = true;
                    else if (cur.gtd * (br[hi].t - br[lo].t) >= 0) br[hi] = br[lo];
                    br[lo] = cur;
                }
            }
            if (n_br == 1) lo = 0;
            t = br[lo].t;
            loss = br[lo].f;
            base = br[lo].k;                                                  // gradient at the accepted point
            be.accept(t);
            const bool opt_cond = slot_gmax[base] <= o.tolerance_grad;        // (no evaluation writes the slot of x: also right for t = 0)
            evals += ls_evals;

            if (n_iter == o.max_iter) break;
            if (evals >= o.max_eval) break;
            if (opt_cond) break;
            if (d_max * std::fabs(t) <= o.tolerance_change) break;
            if (std::fabs(loss - prev_loss) < o.tolerance_change) break;
        }
        res.n_iter = n_iter; res.n_eval = evals; res.loss = loss;
        return be.flush();
    }
};

}  // namespace rc
