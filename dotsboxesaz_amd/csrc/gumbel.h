// gumbel.h -- Gumbel root search (Danihelka et al., ICLR 2022, "Policy improvement by planning with Gumbel"): candidates by
// Gumbel-top-m, the read budget spent by sequential halving, and softmax(logits + sigma(completed Q)) as the policy target, at the
// root of the self-play driver's searches.  The rule is stated in full in include/dbaz.h next to dbaz_selfplay_set_gumbel; this
// file is that statement as code, once, for the preparation (tree.hip: gumbel_prep), the descent (tree.hip: descend), the driver's
// move and row (tree.hip: advance_one) and the host (dbaz_gumbel_considered, dbaz_gumbel_target).
//
// Every expression is float64 in the order written there.  Nothing here may be contracted into a fused multiply-add: tree.hip is
// built with -ffp-contract=off, and the host side targets baseline x86-64, which has none.
// Plain C++ for g++ and hipcc alike.
#pragma once
#include <math.h>
#include <stdint.h>

#include "forced_playouts.h" // FORCED_HD, forced_value (the descent's value_score), FORCED_PRIOR, the SEARCH_* bits below 8

#define SEARCH_GUMBEL 8 // Slot::fast_search: a search of the driver with the Gumbel rule at its root (beside SEARCH_FAST)
#define SEARCH_GUMBEL_FULL 16 // ... in the full mode of the searching model (beside SEARCH_GUMBEL; only the <2> instantiations look at it)

#define GUMBEL_M_MAX 256         // DBAZ_MAX_A (engine.hip asserts it): the most children a root has
#define GUMBEL_C_VISIT_MAX 1e6
#define GUMBEL_C_SCALE_MAX 1e3
#define GUMBEL_LOGIT_MIN (-1e30) // logit of a candidate whose prior is 0 (only when no valid child has a positive prior)
#define GUMBEL_TAG 0x44444444u   // word 3 of the Philox counter of g(a); 0x11111111, 0x22222222, 0x33333333, 0x40000000 and the two
                                 // families 0x80000000 + i, 0xC0000000 + i are the other streams'
#define GUMBEL_PI_ONE 16777216.0 // 2^24: the row's visits are floor(pi' * 2^24 + 0.5)

// u in [2^-53, 1 - 2^-53] -> g = -log(-log(u))
FORCED_HD inline double gumbel_clamp_u(double u)
{
    const double lo = 1.0 / 9007199254740992.0;
    if (u < lo) u = lo;
    if (u > 1.0 - lo) u = 1.0 - lo;
    return u;
}
FORCED_HD inline double gumbel_from_u(double u) { return -log(-log(gumbel_clamp_u(u))); }

FORCED_HD inline double gumbel_logit(double P) { return P > 0.0 ? log(P) : GUMBEL_LOGIT_MIN; }

// gl of a candidate: one product, then one sum.  g_scale = 1.0 (self-play) leaves g's bits; 0.0 is the deterministic search
FORCED_HD inline double gumbel_noisy_logit(double g_scale, double gv, double logit) { return (g_scale * gv) + logit; }

// mctx's sequence of considered visits at position t, in closed form per phase (integers only)
FORCED_HD inline int gumbel_considered(int m_eff, int R, int t)
{
    if (m_eff <= 1) return t;
    int L = 0;
    while ((1 << L) < m_eff) L++; // ceil(log2(m'))
    int nc = m_eff, base = 0, pos = 0;
    for (;;) {
        int extra = R / (L * nc);
        if (extra < 1) extra = 1;
        const int len = extra * nc;
        if (t < pos + len) return base + (t - pos) / nc;
        pos += len;
        base += extra;
        nc = nc / 2 < 2 ? 2 : nc / 2;
    }
}

// sigma of a completed Q
FORCED_HD inline double gumbel_sigma(double c_visit, double c_scale, int n_max, double cq)
{
    return ((c_visit + (double)n_max) * c_scale) * cq;
}

FORCED_HD inline double gumbel_vmix(double num, double den) { return den != 0.0 ? num / den : 0.0; }

// the full mode's mixed value of a node (dbaz_selfplay_set_gumbel_mode): anchored on v, the value the node got at its expansion;
// S = the sum of its children's visits
FORCED_HD inline double gumbel_vmix_full(double v, int S, double num, double den)
{
    return den != 0.0 ? (v + (double)S * (num / den)) / (1.0 + (double)S) : v;
}

// the full mode's score of a candidate below the root: pi'(a) - n(a) / (1 + S)
FORCED_HD inline double gumbel_nonroot_score(double pi, int n, int S) { return pi - (double)n / (1.0 + (double)S); }

// the row's count of a target probability
FORCED_HD inline int32_t gumbel_count(double pi) { return (int32_t)floor(pi * GUMBEL_PI_ONE + 0.5); }

// ---- host side ------------------------------------------------------------------------------------------------------------
// the sum order of the rule: lane i of 64 adds its entries i, i + 64, i + 128, i + 192 (absent ones +0.0), then six butterfly
// stages s = s + s[lane ^ o], o = 32 .. 1.  Every lane ends with the same bits; lane 0's are returned.
inline double gumbel_sum(const double *x, int n)
{
    double s[64], t[64];
    for (int l = 0; l < 64; l++) {
        double a = 0.0;
        for (int i = l; i < 256; i += 64) a = a + (i < n ? x[i] : 0.0);
        s[l] = a;
    }
    for (int o = 32; o > 0; o >>= 1) {
        for (int l = 0; l < 64; l++) t[l] = s[l] + s[l ^ o];
        for (int l = 0; l < 64; l++) s[l] = t[l];
    }
    return s[0];
}

// pi'(a) = softmax(logit + sigma(completed Q)) over the candidates of one node, 0.0 for every other child; full: the completed Q
// of an unvisited child is the full v_mix around v, else the root-only one (v is not read).  Returns S; cand_out may be null.
inline int gumbel_policy_row(int n_actions, double c_visit, double c_scale, bool full, double v, const double *P, const float *W,
                             const uint32_t *ns, const uint8_t *valid, double *pi, bool *cand_out)
{
    double a[GUMBEL_M_MAX], b[GUMBEL_M_MAX], x[GUMBEL_M_MAX];
    bool cand[GUMBEL_M_MAX];
    bool any = false;
    int n_max = 0, S = 0;
    for (int i = 0; i < n_actions; i++) {
        const int n = (int)(ns[i] & FORCED_VISITS_MASK);
        a[i] = b[i] = 0.0;
        if (n > 0) {
            a[i] = P[i] * forced_value(W[i], n, (ns[i] & FORCED_SAME_BIT) != 0);
            b[i] = P[i];
        }
        S += n;
        if (valid[i] && n > n_max) n_max = n;
        if (valid[i] && P[i] > 0.0) any = true;
    }
    const double num = gumbel_sum(a, n_actions), den = gumbel_sum(b, n_actions);
    const double vmix = full ? gumbel_vmix_full(v, S, num, den) : gumbel_vmix(num, den);
    double M = -INFINITY;
    for (int i = 0; i < n_actions; i++) {
        const int n = (int)(ns[i] & FORCED_VISITS_MASK);
        cand[i] = valid[i] && (P[i] > 0.0 || !any);
        if (cand_out) cand_out[i] = cand[i];
        if (!cand[i]) continue;
        const double cq = n > 0 ? forced_value(W[i], n, (ns[i] & FORCED_SAME_BIT) != 0) : vmix;
        x[i] = gumbel_logit(P[i]) + gumbel_sigma(c_visit, c_scale, n_max, cq);
        if (x[i] > M) M = x[i];
    }
    for (int i = 0; i < n_actions; i++) a[i] = cand[i] ? exp(x[i] - M) : 0.0;
    const double se = gumbel_sum(a, n_actions);
    for (int i = 0; i < n_actions; i++) pi[i] = cand[i] ? a[i] / se : 0.0;
    return S;
}

// the whole target on one root (the host's dbaz_gumbel_target and dbaz_gumbel_target_full): out[i] = the row's visits of child i
inline void gumbel_target_row(int n_actions, double c_visit, double c_scale, const double *P, const float *W, const uint32_t *ns,
                              const uint8_t *valid, int32_t *out, bool full = false, double v = 0.0)
{
    double pi[GUMBEL_M_MAX];
    bool cand[GUMBEL_M_MAX];
    gumbel_policy_row(n_actions, c_visit, c_scale, full, v, P, W, ns, valid, pi, cand);
    for (int i = 0; i < n_actions; i++) out[i] = cand[i] ? gumbel_count(pi[i]) : 0;
}

// the full mode's pick below the root (the host's dbaz_gumbel_nonroot_pick): the first maximum of pi'(a) - n(a) / (1 + S) over the
// candidates
inline int gumbel_nonroot_pick_row(int n_actions, double c_visit, double c_scale, double v, const double *P, const float *W,
                                   const uint32_t *ns, const uint8_t *valid)
{
    double pi[GUMBEL_M_MAX];
    bool cand[GUMBEL_M_MAX];
    const int S = gumbel_policy_row(n_actions, c_visit, c_scale, true, v, P, W, ns, valid, pi, cand);
    int best = -1;
    double bs = -INFINITY;
    for (int i = 0; i < n_actions; i++) {
        if (!cand[i]) continue;
        const double sc = gumbel_nonroot_score(pi[i], (int)(ns[i] & FORCED_VISITS_MASK), S);
        if (best < 0 || sc > bs) { bs = sc; best = i; }
    }
    return best;
}
