// forced_playouts.h -- forced playouts and policy target pruning (Wu 2019, "Accelerating Self-Play Learning in Go", section 3.2)
// at the root of the self-play driver's full searches.  The rule is stated in full in include/dbaz.h next to
// dbaz_selfplay_set_forced_playouts; this file is that statement as code, once, for the descent (tree.hip: descend), the
// driver's row (tree.hip: advance_one) and the host (dbaz_prune_visits).
//
// Every expression is float64 in the order written there.  Nothing here may be contracted into a fused multiply-add: tree.hip is
// built with -ffp-contract=off, and the host side targets baseline x86-64, which has none.
// Plain C++ for g++ and hipcc alike.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FORCED_HD __host__ __device__
#else
#define FORCED_HD
#endif

#define FORCED_K_MAX 16.0
#define FORCED_SCORE 1e20 // the score of a forced child in the descent's argmax
// descend (tree.hip) gives the lowest forced child this root prior instead: pb_c * FORCED_PRIOR is finite and above FORCED_SCORE
// for every pb_c a search can have (pb_c >= cpuct / (n + 1) with n < 2^30), so the argmax takes that child, as the rule has it
#define FORCED_PRIOR 1e300

// Slot::fast_search, the kind of the slot's current search (begin_search writes it): bit 0 is the playout cap's
#define SEARCH_FAST 1   // a fast search of the playout cap (playout_cap.h)
#define SEARCH_FORCED 2 // a full search of the self-play driver with forced playouts at its root
#define SEARCH_PRUNE 4  // ... whose row records the pruned visits (ROW_FLAG_PRUNED)

// a child's visits | same-player bit, as the tree keeps them (common.h: NS_MASK, NS_SAME)
#define FORCED_VISITS_MASK 0x3FFFFFFFu
#define FORCED_SAME_BIT 0x40000000u

// the child is forced: visited, and fewer than sqrt(k P N) times
FORCED_HD inline bool forced_child(double k, double P, int n, long long N)
{
    const double t = k * P * (double)N;
    return n > 0 && (double)n * (double)n < t;
}

// the smallest integer f >= 0 with f * f >= k P N
FORCED_HD inline long long forced_count(double k, double P, long long N)
{
    const double t = k * P * (double)N;
    if (!(t > 0.0)) return 0;
    long long f = (long long)sqrt(t);
    while ((double)f * (double)f < t) f++;
    while (f > 0 && (double)(f - 1) * (double)(f - 1) >= t) f--;
    return f;
}

// the two terms of the descent's score (children_ucb_score), a child at m visits in the exploration term
FORCED_HD inline double forced_value(float W, int n, bool same)
{
    const double v = (double)W / (double)(1 + n);
    return v * (same ? 1.0 : -1.0);
}
FORCED_HD inline double forced_expl(double pbc, double sq, long long m, double P)
{
    const double t = sq / (double)(m + 1);
    const double pb_c = pbc * t;
    return pb_c * P;
}

// U* of the most visited child
FORCED_HD inline double forced_ustar(double pbc, double sq, double P, float W, uint32_t ns)
{
    const int n = (int)(ns & FORCED_VISITS_MASK);
    return forced_expl(pbc, sq, n, P) + forced_value(W, n, (ns & FORCED_SAME_BIT) != 0);
}

// n' of a valid child other than c*: the smallest m in [max(0, n - f), n] with expl(c, m) + value(c) < U*, n if there is none,
// and 0 instead of a single playout left by a cut.  The predicate is monotone in m (a quotient, two products and a sum of
// correctly rounded operations, each monotone in its operand): bisection finds what a scan finds.
FORCED_HD inline int forced_pruned(double k, double pbc, double sq, long long N, double P, float W, uint32_t ns, double ustar)
{
    const int n = (int)(ns & FORCED_VISITS_MASK);
    if (n <= 0) return n;
    const double v = forced_value(W, n, (ns & FORCED_SAME_BIT) != 0);
    const long long f = forced_count(k, P, N);
    long long lo = (long long)n - f;
    if (lo < 0) lo = 0;
    if (!(forced_expl(pbc, sq, n, P) + v < ustar)) return n; // not even at n: nothing to take back
    long long hi = n; // the predicate holds at hi
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (forced_expl(pbc, sq, mid, P) + v < ustar) hi = mid;
        else lo = mid + 1;
    }
    int np = (int)hi;
    if (np < n && np == 1) np = 0;
    return np;
}

// c*: the first valid child with the maximum visit count (-1 without a valid child)
inline int forced_best(int n_actions, const uint32_t *ns, const uint8_t *valid)
{
    int best = -1, bn = -1;
    for (int i = 0; i < n_actions; i++) {
        const int n = (int)(ns[i] & FORCED_VISITS_MASK);
        if (valid[i] && n > bn) { bn = n; best = i; }
    }
    return best;
}

// the whole rule on one root (the host's dbaz_prune_visits): out[i] = n' of child i; an invalid child keeps its count
inline void forced_prune_row(int n_actions, double k, double pbc, double sq, long long N, const double *P, const float *W,
                             const uint32_t *ns, const uint8_t *valid, int32_t *out)
{
    for (int i = 0; i < n_actions; i++) out[i] = (int32_t)(ns[i] & FORCED_VISITS_MASK);
    const int cs = forced_best(n_actions, ns, valid);
    if (cs < 0 || !(k > 0.0)) return;
    const double ustar = forced_ustar(pbc, sq, P[cs], W[cs], ns[cs]);
    for (int i = 0; i < n_actions; i++)
        if (valid[i] && i != cs) out[i] = forced_pruned(k, pbc, sq, N, P[i], W[i], ns[i], ustar);
}
