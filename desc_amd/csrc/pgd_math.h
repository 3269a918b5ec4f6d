// Device arithmetic shared by the sweep kernels of sweep_gather.hip, sweep_node.hip and sweep_band.hip (one problem per handle) and batch.hip (many small problems per launch):
// the plugin step, the simplex projection threshold and the cycle-inconsistency trace.  Both files must produce the same bits
// from the same inputs, so the text lives here once.
#pragma once
#include <cmath>

#include "device_utils.h"

namespace desc {

struct StepArgs {
    const double* adam_m;                 // HybridGradient.m_t / v_t before this GetStep call ...
    const double* adam_v;
    double* adam_m_out;                   // ... and after it: double-buffered like w, because the stop decision for
    double* adam_v_out;                   // iteration t falls during sweep t+1, whose update must be discardable
    double step;                          // step size of this GetStep call
    double lr, beta1, beta2, bc1, bc2;    // Adam (HybridGradient.m:28-35)
};

// The built-in plugins' GetStep call number tp (host): step size and Adam bias corrections into s, whose moment pointers are the
// caller's.  Returns whether the sweep runs the Adam update (HybridGradient, strategy 0).
inline bool plugin_step(const desc_params& p, int tp, StepArgs& s) {
    s.lr = p.lr; s.beta1 = p.beta1; s.beta2 = p.beta2; s.bc1 = 1.0; s.bc2 = 1.0;
    s.step = p.lr;
    if (p.step_kind == DESC_STEP_PIECEWISE) {
        s.step = p.lr / (std::trunc((double)tp / p.decay_interval) + 1.0);            // PiecewiseStepSize.m:16
    } else if (p.step_kind == DESC_STEP_HYBRID) {
        if (p.hybrid_strategy == 0) {
            s.bc1 = 1.0 - std::pow(p.beta1, (double)tp);                             // HybridGradient.m:32-33
            s.bc2 = 1.0 - std::pow(p.beta2, (double)tp);
            return true;
        }
        s.step = 100.0 * (p.lr / (std::trunc((double)tp / p.decay_interval) + 1.0));   // HybridGradient.m:39
    }
    return false;
}

__device__ __forceinline__ double abs_acos_ext(double x) {
    // MATLAB abs(acos(x)) with the complex extension outside [-1,1] (DESC_PGD.m:147)
    if (x > 1.0) return acosh(x);
    if (x < -1.0) return hypot(M_PI, acosh(-x));
    return acos(x);
}

template <int STEP>
__device__ __forceinline__ double apply_step(const StepArgs& a, double w, double g, int64_t c) {
    if (STEP == DESC_STEP_HYBRID) {               // HybridGradient.m:28-35 (strategy 0)
        double mt = (a.beta1 * a.adam_m[c]) + (1.0 - a.beta1) * g;
        double vt = (a.beta2 * a.adam_v[c]) + (1.0 - a.beta2) * (g * g);
        a.adam_m_out[c] = mt; a.adam_v_out[c] = vt;
        double cm = mt / a.bc1, cv = vt / a.bc2;
        return w + (-a.lr * cm / (sqrt(cv) + 1e-8));
    }
    return w + (-a.step * g);                     // ConstantStepSize.m:10 / PiecewiseStepSize.m:17
}

// Simplex projection threshold (DESC_PGD.m:215-223) for one segment held one value per
// lane in a group of G lanes: T with sum(max(ws - T, 0)) = 1.  Michelot's fixed point
// reaches the same active set as the reference's sort-and-scan (the first sorted i with
// sum(w(i:end)-w(i)) < 1).
template <int G>
__device__ __forceinline__ double simplex_threshold(double ws, bool act0, int lane) {
    bool act = act0;
    double T = 0.0;
    for (;;) {
        const double s = group_sum<G>(act ? ws : 0.0);
        const int na = group_count<G>(act, lane);
        T = (s - 1.0) / (double)max(na, 1);
        const bool keep = act && (ws > T);
        const bool changed = keep != act;
        act = keep;
        if (!__any(changed)) break;
    }
    return T;
}

// product-of-three trace in the reference's accumulation order (DESC_PGD.m:137-146)
__device__ __forceinline__ double cycle_trace(const double* A, const double* pb, bool tb, const double* pc, bool tc) {
    double Bm[9], Cm[9], B[9], C[9];
    load_block9(pb, Bm); load_block9(pc, Cm);
    for (int r = 0; r < 3; ++r)
        for (int s = 0; s < 3; ++s) {
            B[r + 3 * s] = tb ? Bm[s + 3 * r] : Bm[r + 3 * s];
            C[r + 3 * s] = tc ? Cm[s + 3 * r] : Cm[r + 3 * s];
        }
    double tr = 0.0;
    for (int r = 0; r < 3; ++r) {
        double P[3];
        for (int s = 0; s < 3; ++s) {
            double acc = 0.0;
            for (int u = 0; u < 3; ++u) acc = acc + A[r + 3 * u] * B[u + 3 * s];
            P[s] = acc;
        }
        double acc = 0.0;
        for (int u = 0; u < 3; ++u) acc = acc + P[u] * C[u + 3 * r];
        tr = tr + acc;
    }
    return tr;
}

}  // namespace desc
