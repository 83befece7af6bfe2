// sgm_wta.hpp -- the winner-take-all (ref :374-443), once, for every kernel that ends a cost sum:
//   sgm_sum_wta_lr_k (sgm_sum_wta.hip), sgm_upsum_k (sgm_upsum.hip): wta_pair_keys, wta_best2, wta_diag_keys, wta_views, wta_finish
//   sgm_sum_wta_k (sgm_sum_wta.hip): keys from its acc[], wta_best2, an OR-reduce for S[best +- 1] (it has no ring), wta_finish
//   sgm_wta_right_k (sgm_sum_wta.hip): serial, wta_feed + wta_finish
// A pixel's disparities lie across the LPP lanes of a DPP row, DPL per lane; key = S << 16 | d, so the row-wide minimum key
// is the first minimum the reference's strict '>' finds (ref :390).

#pragma once
#include "sgm_common.hpp"

// a * b + c for a, b < 2^24: v_mad_u32_u24 (half rate); hipcc turns the plain 32-bit form into v_mad_u64_u32 / v_mul_lo_u32
static __device__ __forceinline__ unsigned umad24(unsigned a, unsigned b, unsigned c) { return __umul24(a, b) + c; }

struct WtaState {
    unsigned m1, m2;   // smallest cost (lowest d wins ties, ref :390) and smallest among the others (ref :413-419)
    int d1;            // index (d - dmin) of m1, -1 if nothing beat 65535
    unsigned c1, c2;   // cost_local[best-1], cost_local[best+1] (ref :432-435)
    unsigned pv;       // cost of the previous index
    bool want_next;
};

static __device__ __forceinline__ void wta_feed(WtaState& s, unsigned v, int di)
{
    if (s.want_next) { s.c2 = v; s.want_next = false; }
    if (v < s.m1) {
        s.m2 = s.m1; s.m1 = v; s.d1 = di; s.c1 = s.pv; s.want_next = true; s.c2 = 0xFFFFu;
    } else if (v < s.m2) {
        s.m2 = v;
    }
    s.pv = v;
}

static __device__ __forceinline__ float wta_finish(const WtaState& s, int D, int dmin, int check_unique, float one_minus_ratio)
{
    const float inf = __builtin_inff();
    if (s.d1 < 0) return inf;                             // no candidate at all (see oracle/sgm_oracle.c sgmo_wta)
    if (check_unique) {                                   // ref :412-426 (Q10)
        const unsigned margin = (unsigned)(unsigned short)(int)((float)s.m1 * one_minus_ratio);
        if ((int)s.m2 - (int)s.m1 <= (int)margin) return inf;
    }
    if (s.d1 == 0 || s.d1 == D - 1) return inf;          // ref :428
    const int c1 = (int)(short)s.c1, c2 = (int)(short)s.c2;       // (int16_t) casts, 65535 -> -1 (Q11b)
    int denom = (int)(short)(c1 + c2 - 2 * (int)s.m1);
    if (denom < 1) denom = 1;
    return (float)(s.d1 + dmin) + (float)(c1 - c2) / ((float)denom * 2.0f);     // ref :440
}

// OR over the 16 lanes of a DPP row, result in every lane
static __device__ __forceinline__ unsigned row_allor(unsigned v)
{
    v |= dpp_perm<DPP_QUAD_XOR1>(v);
    v |= dpp_perm<DPP_QUAD_XOR2>(v);
    v |= dpp_perm<DPP_ROW_HALF_MIRROR>(v);
    v |= dpp_perm<DPP_ROW_MIRROR>(v);
    return v;
}

// matching confidence from the best and runner-up cost (include/sgm_mi355x.h): 0 for a tie or no candidate; one u32 divide
static __device__ __forceinline__ uint16_t conf_value(unsigned m1, unsigned m2)
{
    return m2 == 0u ? (uint16_t)0 : (uint16_t)(((m2 - m1) * 65535u) / m2);
}

// keys of a lane's DPL disparities from its S pairs in disparity order, pr[m] = (S(2m), S(2m+1)); padding disparities carry
// 65535 (the caller ORed it in), so their keys lose against every real one.  Returns the lane's smallest key.
template <int DPL>
static __device__ __forceinline__ unsigned wta_pair_keys(const unsigned (&pr)[DPL / 2], int sub, unsigned (&key)[DPL])
{
    unsigned kmin = 0xFFFFFFFFu;
#pragma unroll
    for (int m = 0; m < DPL / 2; ++m) {
        const unsigned idx = (unsigned)(sub * DPL + 2 * m);
        key[2 * m] = (pr[m] << 16) | idx;
        key[2 * m + 1] = (pr[m] & 0xFFFF0000u) | (idx + 1);
        kmin = min(kmin, min(key[2 * m], key[2 * m + 1]));
    }
    return kmin;
}

// best and runner-up key of the pixel, in every one of its LPP lanes.  The best key is unique (it carries its d), so
// key - kbest - 1 (mod 2^32) sends it to the top and keeps the order of all others: 0xFFFFFFFF comes back when there is no
// other disparity, as ref :381.
template <int DPL, int LPP>
static __device__ __forceinline__ void wta_best2(const unsigned (&key)[DPL], unsigned kmin, unsigned& kbest, unsigned& ksecond)
{
    kbest = row_allmin<LPP>(kmin);
    const unsigned nbest = ~kbest;
    unsigned k2 = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < DPL; ++i) k2 = min(k2, key[i] + nbest);
    ksecond = row_allmin<LPP>(k2) + kbest + 1;
}

// keys of the right view (ref :397-408: cost of right pixel xr at disparity d is S[xr+d][d], a diagonal through consecutive
// columns) from a ring u16 [columns][LD] in LDS.  diag = the lane's first entry; the ring's mirror slots keep its DPL columns
// from wrapping, so the gather is immediate offsets.  Padding disparities and columns past the image hold 65535; with `padded`
// (D < the padded range) the padding disparities also reach into slots ahead of the newest column: keys forced to the top.
template <int DPL>
static __device__ __forceinline__ unsigned wta_diag_keys(const unsigned short* diag, int LD, int sub, int D, bool padded, unsigned (&key)[DPL])
{
    unsigned val[DPL];
    unsigned kmin = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < DPL; ++i) val[i] = diag[i * (LD + 1)];
    if (!padded) {                                       // wave-uniform: every slot read was written
#pragma unroll
        for (int i = 0; i < DPL; ++i) {
            key[i] = (val[i] << 16) | (unsigned)(sub * DPL + i);
            kmin = min(kmin, key[i]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < DPL; ++i) {
            const int k = sub * DPL + i;
            key[i] = (k < D) ? ((val[i] << 16) | (unsigned)k) : 0xFFFFFFFFu;
            kmin = min(kmin, key[i]);
        }
    }
    return kmin;
}

// Both views end in ONE wta_finish per iteration (uniqueness test, float divide of the sub-pixel term: ~35 instructions a
// wave pays in full even for a single active lane): lane 0 of a pixel finishes the left view of the column in ring slot
// `slot` (if active_l), lane 1 the right view whose diagonal starts in slot `base` (if active_r).  This gathers that lane's
// state for wta_finish: S[best-1] and S[best+1] come straight from the ring (u16 [R][LD]), the column's own slot for the
// left view, the diagonal for the right one (a best at either end of the range is invalid anyway, ref :428: clamp, value
// unused); right view: nothing beat 65535 -> no candidate (ref :381, strict '>').  The caller works out where the map goes
// and calls wta_finish on st there: with the address computed any earlier or later the three-row sweep spills (NOTES.md 22).
struct WtaViews { bool active, is_r; WtaState st; };      // this lane finishes a view / the right one / its state, if active

static __device__ __forceinline__ WtaViews wta_views(const unsigned short* ring, int R, int LD, int sub, int slot, int base, unsigned kbest_l,
                                                     unsigned ksecond_l, unsigned kbest_r, unsigned ksecond_r, bool active_l, bool active_r, int Dp)
{
    WtaViews v = {};
    v.is_r = (sub == 1);
    v.active = v.is_r ? active_r : (sub == 0 && active_l);
    if (v.active) {
        const unsigned kb = v.is_r ? kbest_r : kbest_l, k2nd = v.is_r ? ksecond_r : ksecond_l;
        const int dbest = (int)(kb & 0xFFFFu);
        const int km = max(dbest - 1, 0), kp = min(dbest + 1, Dp - 1);
        int sm = slot, sp = slot;
        if (v.is_r) {
            sm = base + km; sp = base + kp;
            if (sm >= R) sm -= R;
            if (sp >= R) sp -= R;
        }
        v.st.m1 = kb >> 16;
        v.st.m2 = k2nd >> 16;                            // 0xFFFF if there is no other disparity, as ref :381
        v.st.d1 = (v.is_r && (kb >> 16) == 0xFFFFu) ? -1 : dbest;
        v.st.c1 = ring[umad24((unsigned)sm, (unsigned)LD, (unsigned)km)];
        v.st.c2 = ring[umad24((unsigned)sp, (unsigned)LD, (unsigned)kp)];
    }
    return v;
}
