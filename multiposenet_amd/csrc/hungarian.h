// The optimal assignment that pose_track.hip (detections against tracks) and track_eval.hip (ground truths against tracked
// persons) share: the shortest-augmenting-path Hungarian method of include/mpn.h (under mpn_pose_track_optimal) in 64-bit
// integers, run by ONE wave without LDS writes, barriers or atomics. The weight of an eligible pair is quantum_of(s) + 1 + kBias.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kAssignSide = 64;         // rows and real columns of a problem: one lane of the wave per column and per row

// the quantum of a similarity: floor(s * 2^20) in f64 (the product is exact), clamped before the conversion
constexpr double kQuanta = 1048576.0;
__device__ __forceinline__ long long quantum_of(double s) {
    double q = floor(s * kQuanta);
    q = q < 0.0 ? 0.0 : (q > kQuanta ? kQuanta : q);
    return (long long)q;
}

// The method in 64-bit integers (a cost is at most 2^20 + 1 + kBias in size; a delta is at most the reduced cost of the way
// to row i's own dummy, -u[i] - v[T + i], so the potentials grow by a few costs per row: about 64 * (2^20 + kBias), 2^34 with
// the evaluation's bias of 2^27, far short of the type). One wave; rows 1..n, columns 1..T the real ones, T+1..T+n the rows'
// dummies. sim[row][column] holds the similarities; the pair (row, column) is eligible when the column is `live` and
// sim >= thr (a NaN never is). Lane L owns column L + 1 ("A") and column T + L + 1 (the dummy of row L + 1; "B") - their v,
// minv, way, used and p - and the potential u of row L + 1. What the current column and row decide (j0, i0, delta, the
// tree's rows) is the same value in every lane: a value fetched from its owner by a shuffle, or the outcome of the
// butterfly. Every loop has a compile-time bound: a row whose search or flip does not end within it ends the matching with
// the rows before it (which cannot happen: a search takes a new column into its tree in every trip and there are at most
// 128). On return `mine` is the row on the lane's real column (-1 = none: left as it was) and mine_sim its similarity.
// `rows` (the same value in every lane): bit i - 1 clear leaves row i out. A row without an eligible pair may be left out
// without changing anything: its search ends on its own dummy with delta = 0, so no potential moves and no real column is
// touched; the trips it would take are the only difference.
constexpr int kAssignCols = 2 * kAssignSide;
constexpr long long kAbsent = 1ll << 62;

template <long long kBias>
__device__ __forceinline__ void assign_optimal(const double (*sim)[kAssignSide], int n, int T, int lane, bool live, double thr,
                                               int& mine, double& mine_sim, unsigned long long rows = ~0ull) {
    const int jA = lane < T ? lane + 1 : -1, jB = T + lane + 1;
    long long u = 0, vA = 0, vB = 0;
    int pA = 0, pB = 0;
    for (int i = 1; i <= kAssignSide; ++i) {
        if (i > n) break;
        if (!((rows >> (i - 1)) & 1ull)) continue;         // (uniform) a row the caller knows to have no eligible pair
        long long minvA = kAbsent, minvB = kAbsent;
        int wayA = 0, wayB = 0;
        bool usedA = false, usedB = false, reached = false;
        unsigned long long tree = 0ull;                   // the rows whose column is used (and row i, on column 0)
        int j0 = 0, i0 = i;
        for (int trip = 0; trip <= kAssignCols; ++trip) {
            usedA = usedA || j0 == jA;
            usedB = usedB || j0 == jB;
            tree |= 1ull << (i0 - 1);
            const long long u0 = __shfl(u, i0 - 1, 64);
            if (live && !usedA) {
                const double s = sim[i0 - 1][lane];
                if (s >= thr) {                           // (a NaN is never eligible)
                    const long long cur = -(quantum_of(s) + 1 + kBias) - u0 - vA;
                    if (cur < minvA) { minvA = cur; wayA = j0; }
                }
            }
            if (lane == i0 - 1 && !usedB) {
                const long long cur = -u0 - vB;
                if (cur < minvB) { minvB = cur; wayB = j0; }
            }
            // delta = the smallest minv of the unused columns, ties to the smaller column (jA < jB within a lane)
            long long delta = kAbsent;
            int j1 = -1;
            if (!usedA && minvA != kAbsent) { delta = minvA; j1 = jA; }
            if (!usedB && minvB != kAbsent && (j1 < 0 || minvB < delta)) { delta = minvB; j1 = jB; }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const long long v2 = __shfl_xor(delta, o, 64);
                const int j2 = __shfl_xor(j1, o, 64);
                if (j2 >= 0 && (j1 < 0 || v2 < delta || (v2 == delta && j2 < j1))) { delta = v2; j1 = j2; }
            }
            if (j1 < 0) break;                            // (row i's own dummy is always there; uniform)
            if ((tree >> lane) & 1ull) u += delta;
            if (usedA) vA -= delta; else if (minvA != kAbsent) minvA -= delta;
            if (usedB) vB -= delta; else if (minvB != kAbsent) minvB -= delta;
            j0 = j1;
            const int rowA = __shfl(pA, (j0 - 1) & 63, 64), rowB = __shfl(pB, (j0 - T - 1) & 63, 64);
            i0 = j0 <= T ? rowA : rowB;
            if (i0 < 1 || i0 > n) { reached = i0 == 0; break; }
        }
        if (!reached) break;
        for (int trip = 0; trip <= kAssignCols; ++trip) { // the path back to column 0: every column takes the row before it
            const int wA = __shfl(wayA, (j0 - 1) & 63, 64), wB = __shfl(wayB, (j0 - T - 1) & 63, 64);
            const int j1 = j0 <= T ? wA : wB;
            const int rowA = __shfl(pA, (j1 - 1) & 63, 64), rowB = __shfl(pB, (j1 - T - 1) & 63, 64);
            const int row = j1 == 0 ? i : (j1 <= T ? rowA : rowB);
            if (j0 == jA) pA = row;
            if (j0 == jB) pB = row;
            j0 = j1;
            if (j0 <= 0) break;
        }
    }
    if (live && pA >= 1 && pA <= n) { mine = pA - 1; mine_sim = sim[mine][lane]; }
}

}  // namespace
