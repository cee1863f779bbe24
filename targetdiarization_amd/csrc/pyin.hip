// pyin.hip — probabilistic YIN pitch tracking on MI355X: the body of the reference's ASRProcessor.f0_compute
// (ASRProcessor.py:1003-1010, `librosa.pyin(audio, fmin=fmin, fmax=fmax, sr=sampling_rate)`; third-party algorithm, restated from
// upstream — DESIGN 8.21).  One call tracks every clip of a packed buffer; the host describes a clip by a table entry of 4 int64:
//     [0] off     packed-input index of the clip's sample 0          [1] n   samples of the clip
//     [2] frame0  first row of the clip in the per-frame planes      [3] T   frames of the clip
// Three launches whatever the number of clips:
//     pyin_yin_kernel      one workgroup per frame: the frame in LDS (zero outside the clip), the difference function
//                          d[tau] = sum_{j=1..W} (y[j] - y[j+tau])^2 summed directly in fp32 (eight strided partial sums, combined
//                          pairwise), the cumulative mean through a workgroup prefix sum, the parabolic shifts
//     pyin_obs_kernel      one workgroup per frame: troughs compacted in order of period, the first threshold each lies below, the
//                          Boltzmann-weighted sum over thresholds in fp64 in ascending order, one thread per trough; the pitch bin
//                          of a candidate, the candidate of the longest period per bin (an integer max in LDS, no float atomics),
//                          the voiced probability by a fixed-order tree
//     pyin_viterbi_kernel  one workgroup per clip, sequential over frames, one barrier per frame; fp64 scores double-buffered in
//                          LDS behind -inf halos, the log triangle in LDS, two lanes per pitch bin (half a band each), uint16
//                          back-pointers in the workspace, the backtrack by one lane
// The Viterbi transition matrix is banded (triangle of `width` bins around the source, each source row normalised on its own);
// outside the band upstream's log(0 + tiny) is finite, so every destination also considers max_k value[k] + log(tiny) with that
// first global argmax as its pointer: inside the band the real transition beats it, outside it is the dense matrix's own candidate.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "../../include/tdx.h"
#include "tdx_common.hpp"

using namespace tdx;

namespace {

constexpr int TAB = 4;
constexpr int MAX_FRAME = 8192, MAX_PERIOD = 4096, MAX_STATES = 4096, MAX_THRESH = 254, MAX_CLIPS = 65535;
constexpr int OBS_THREADS = 256, VIT_MAX_THREADS = 1024, VIT_MAX_WAVES = VIT_MAX_THREADS / 64;
constexpr float TINY_F = 1.17549435e-38f;
constexpr double TINY_D = 2.2250738585072014e-308;

struct Clip { long off, n, frame0; int T; };
__device__ __forceinline__ Clip load_clip(const long* __restrict__ tab, int c) {
    const long* t = tab + (long)c * TAB;
    Clip k;
    k.off = t[0]; k.n = t[1]; k.frame0 = t[2]; k.T = (int)t[3];
    return k;
}

// inclusive prefix sum over the n threads of the workgroup (fixed order: Hillis-Steele through LDS)
template <typename T>
__device__ __forceinline__ T block_scan(T v, T* buf, int tid, int n) {
    buf[tid] = v;
    __syncthreads();
    for (int o = 1; o < n; o <<= 1) {
        const T a = tid >= o ? buf[tid - o] : T(0);
        __syncthreads();
        buf[tid] += a;
        __syncthreads();
    }
    return buf[tid];
}

struct YinArgs {
    const float* x; const long* tab;
    int frame_length, W, hop, pad, min_period, max_period;
    float* yin; float* shifts;                 // [frames][n_lags]
};

// grid (max frames of a clip, clips); LDS: frame[frame_length] | d[max_period + 1] | part[threads]
__global__ __launch_bounds__(1024) void pyin_yin_kernel(YinArgs p) {
    extern __shared__ float ysm[];
    const Clip c = load_clip(p.tab, blockIdx.y);
    const int t = blockIdx.x;
    if (t >= c.T) return;
    const int tid = threadIdx.x, nt = blockDim.x;
    float* fr = ysm;
    float* d = fr + p.frame_length;
    float* part = d + p.max_period + 1;
    const long s0 = (long)t * p.hop - p.pad;
    for (int i = tid; i < p.frame_length; i += nt) {
        const long s = s0 + i;
        fr[i] = (s >= 0 && s < c.n) ? p.x[c.off + s] : 0.f;
    }
    __syncthreads();
    const int W = p.W, W8 = W & ~7;
    for (int tau = 1 + tid; tau <= p.max_period; tau += nt) {
        float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const float* y0 = fr + 1;
        const float* y1 = fr + 1 + tau;
        for (int j = 0; j < W8; j += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) { const float e = y0[j + u] - y1[j + u]; a[u] = fmaf(e, e, a[u]); }
        }
        for (int j = W8; j < W; ++j) { const float e = y0[j] - y1[j]; a[j - W8] = fmaf(e, e, a[j - W8]); }
        d[tau] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    }
    __syncthreads();
    // cumulative mean: thread `tid` owns the lags 1 + tid L .. tid L + L
    const int L = (p.max_period + nt - 1) / nt;
    const int lo = 1 + tid * L, hi = min(p.max_period, tid * L + L);
    float s = 0.f;
    for (int tau = lo; tau <= hi; ++tau) s += d[tau];
    float run = block_scan(s, part, tid, nt) - s;
    for (int tau = lo; tau <= hi; ++tau) {
        run += d[tau];
        if (tau >= p.min_period) d[tau] = d[tau] / (run / (float)tau + TINY_F);
    }
    __syncthreads();
    const int n_lags = p.max_period - p.min_period + 1;
    const float* v = d + p.min_period;
    const long o = (c.frame0 + t) * (long)n_lags;
    for (int r = tid; r < n_lags; r += nt) {
        float sh = 0.f;
        if (r > 0 && r < n_lags - 1) {
            const float xm = v[r - 1], x0 = v[r], xp = v[r + 1];
            const float a = (xm + xp) - 2.f * x0;
            const float b = (xp - xm) * 0.5f;
            if (fabsf(b) < fabsf(a)) sh = -b / a;
        }
        p.yin[o + r] = v[r];
        p.shifts[o + r] = sh;
    }
}

struct ObsArgs {
    const float* yin; const float* shifts; const long* tab;
    const double *thr, *beta, *beta_cum, *bfact, *bexp;
    int n_lags, npb, nth, min_period;
    double sr, fmin, bins_per_octave, no_trough_prob;
    float* obs; float* voiced_prob;            // [frames][2 npb], [frames]
};

inline size_t obs_lds_bytes(int n_lags, int npb, int nth) {
    return (size_t)OBS_THREADS * 8 + (size_t)n_lags * 4 + (size_t)npb * 4 + (size_t)(npb + 1) * 4 + (size_t)OBS_THREADS * 4 + (size_t)(nth + 2) * 4 + 4 * 4 +
           (size_t)n_lags * 2 * 2 + (size_t)n_lags;
}

// grid (max frames of a clip, clips)
__global__ __launch_bounds__(OBS_THREADS) void pyin_obs_kernel(ObsArgs p) {
    extern __shared__ double osm[];
    const Clip c = load_clip(p.tab, blockIdx.y);
    const int t = blockIdx.x;
    if (t >= c.T) return;
    const int tid = threadIdx.x, n_lags = p.n_lags, npb = p.npb, nth = p.nth;
    double* red = osm;                                   // [256]
    float* x = (float*)(red + OBS_THREADS);              // [n_lags] heights by row
    float* col = x + n_lags;                             // [npb]
    int* win = (int*)(col + npb);                        // [npb + 1] the longest-period row that falls into the bin
    int* scan = win + npb + 1;                           // [256]
    int* cnt = scan + OBS_THREADS;                       // [nth + 2] troughs below threshold k
    int* misc = cnt + nth + 2;                           // [4]: the lowest trough
    unsigned short* tro = (unsigned short*)(misc + 4);   // [n_lags] row of trough c
    unsigned short* cbin = tro + n_lags;                 // [n_lags] bin of trough c
    unsigned char* kk = (unsigned char*)(cbin + n_lags); // [n_lags] first threshold trough c lies below (nth + 1: none)
    const long frame = c.frame0 + t;
    const float* yr = p.yin + frame * n_lags;
    const float* sr_ = p.shifts + frame * n_lags;
    for (int i = tid; i < n_lags; i += OBS_THREADS) x[i] = yr[i];
    for (int i = tid; i < npb; i += OBS_THREADS) col[i] = 0.f;
    for (int i = tid; i <= npb; i += OBS_THREADS) win[i] = -1;
    __syncthreads();
    // troughs, compacted in order of period: thread `tid` owns the rows tid L .. tid L + L - 1
    const int L = (n_lags + OBS_THREADS - 1) / OBS_THREADS;
    const int lo = tid * L, hi = min(n_lags, lo + L);
    auto is_trough = [&](int i) {
        if (i == 0) return x[0] < x[1];
        if (i == n_lags - 1) return x[i] < x[i - 1];
        return x[i] < x[i - 1] && x[i] <= x[i + 1];
    };
    int mine = 0;
    for (int i = lo; i < hi; ++i) mine += is_trough(i) ? 1 : 0;
    int at = block_scan(mine, scan, tid, OBS_THREADS) - mine;
    const int ntro = scan[OBS_THREADS - 1];
    for (int i = lo; i < hi; ++i)
        if (is_trough(i)) {
            const double h = (double)x[i];
            int k = 1;
            while (k <= nth && !(h < p.thr[k])) ++k;
            tro[at] = (unsigned short)i; kk[at] = (unsigned char)k;
            ++at;
        }
    __syncthreads();
    if (tid >= 1 && tid <= nth) {
        int n = 0;
        for (int q = 0; q < ntro; ++q) n += kk[q] <= tid ? 1 : 0;
        cnt[tid] = n;
    }
    if (tid == OBS_THREADS - 1) {                        // the lowest trough, the first one on ties
        int best = -1; float bh = 0.f;
        for (int q = 0; q < ntro; ++q) { const float h = x[tro[q]]; if (best < 0 || h < bh) { best = q; bh = h; } }
        misc[0] = best;
    }
    __syncthreads();
    const int gmin = misc[0];
    float pr[(MAX_PERIOD + OBS_THREADS - 1) / OBS_THREADS];      // the probability of trough tid + 256 it
#pragma unroll
    for (int it = 0; it < (MAX_PERIOD + OBS_THREADS - 1) / OBS_THREADS; ++it) {
        const int q = tid + it * OBS_THREADS;
        if (q >= ntro) break;
        const int k0 = kk[q];
        double prob = 0.0;
        for (int k = k0; k <= nth; ++k) {
            int pos = 0;
            for (int r = 0; r < q; ++r) pos += kk[r] <= k ? 1 : 0;
            prob += (p.bfact[cnt[k]] * p.bexp[pos]) * p.beta[k - 1];
        }
        if (q == gmin) prob += p.no_trough_prob * p.beta_cum[k0 - 1];
        int bin = npb;
        if (prob != 0.0) {
            const int row = tro[q];
            const double period = (double)(p.min_period + row) + (double)sr_[row];
            const double f0 = p.sr / period;
            const double bf = rint(p.bins_per_octave * log2(f0 / p.fmin));          // round half to even
            bin = bf > (double)npb ? npb : (bf >= 0.0 ? (int)bf : 0);
            if (bin < npb) atomicMax(&win[bin], row);
        }
        cbin[q] = (unsigned short)bin;
        pr[it] = (float)prob;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < (MAX_PERIOD + OBS_THREADS - 1) / OBS_THREADS; ++it) {
        const int q = tid + it * OBS_THREADS;
        if (q >= ntro) break;
        const int bin = cbin[q];
        if (bin < npb && win[bin] == (int)tro[q]) col[bin] = pr[it];
    }
    __syncthreads();
    double s = 0.0;
    for (int i = tid; i < npb; i += OBS_THREADS) s += (double)col[i];
    red[tid] = s;
    __syncthreads();
    for (int o = OBS_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const double vp = fmin(fmax(red[0], 0.0), 1.0);
    const float unv = (float)((1.0 - vp) / (double)npb);
    float* orow = p.obs + frame * 2L * npb;
    for (int i = tid; i < npb; i += OBS_THREADS) { orow[i] = col[i]; orow[npb + i] = unv; }
    if (tid == 0) p.voiced_prob[frame] = (float)vp;
}

struct VitArgs {
    const float* obs; const long* tab; long T1;          // tab NULL: one sequence of T1 frames
    int npb, width;
    const double *ltri, *lrow;                           // log triangle [width]; -log of the row sums [npb]
    double l_stay, l_switch, l_init_u, l_tiny;
    unsigned short* ptr; int* states;
    int chunk;                                           // frames per backtrack step (vit_chunk)
};

struct Best { double v; int i; };
__device__ __forceinline__ void take(Best& a, double v, int i) {      // the larger value; on equal values the smaller state
    if (v > a.v || (v == a.v && i < a.i)) { a.v = v; a.i = i; }
}

// LDS of the Viterbi workgroup: U[2][2][npb + 2 hw] (a halo of hw cells of -inf on both sides of each half, so the band loop has no
// range test) | ltri[width] | the waves' best values [2][16] and states [2][16]
inline size_t vit_lds_base(int npb, int width) {
    return ((size_t)4 * (npb + 2 * (width / 2)) + width + 2 * VIT_MAX_WAVES) * 8 + 2 * VIT_MAX_WAVES * 4;
}
// ... | back-pointer rows of the backtrack [chunk][2 npb] uint16: up to 64 frames while the total stays under 60 KB, else one
inline int vit_chunk(int npb, int width) {
    const size_t base = vit_lds_base(npb, width), row = (size_t)4 * npb, pref = base < 60 * 1024 ? 60 * 1024 - base : 0;
    return (int)std::min<size_t>(64, std::max<size_t>(1, pref / row));
}
inline size_t vit_lds_bytes(int npb, int width) { return vit_lds_base(npb, width) + (size_t)vit_chunk(npb, width) * 4 * npb; }

// grid (clips); threads: a multiple of 64 >= min(2 npb, 1024).  Two neighbouring lanes share a pitch bin: each scans one half of the
// band over both source halves, they exchange their maxima through a lane swap, then lane 0 of the pair scores the voiced
// destination of the bin and lane 1 the unvoiced one.  A thread owns the pairs tid, tid + threads, ... (at most VIT_SLOTS).
constexpr int VIT_SLOTS = MAX_STATES / VIT_MAX_THREADS;
__global__ __launch_bounds__(VIT_MAX_THREADS) void pyin_viterbi_kernel(VitArgs p) {
    extern __shared__ double vsm[];
    const int npb = p.npb, S = 2 * npb, hw = p.width / 2, width = p.width, pitch = npb + 2 * hw;
    long frame0 = 0, T = p.T1;
    if (p.tab) { const Clip c = load_clip(p.tab, blockIdx.x); frame0 = c.frame0; T = c.T; }
    if (T < 1) return;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    double* U = vsm;                                     // [2][2][pitch]: value + lrow[bin] of the previous / the current frame
    double* LT = U + 4 * pitch;                          // [width]
    double* wv = LT + width;                             // [2][VIT_MAX_WAVES] the best value of a wave ...
    int* wi = (int*)(wv + 2 * VIT_MAX_WAVES);            // ... and its first state
    const float* obs = p.obs + frame0 * S;
    unsigned short* ptr = p.ptr + frame0 * S;
    int* states = p.states + frame0;
    const double NINF = -HUGE_VAL;
    for (int i = tid; i < 4 * pitch; i += nt) U[i] = NINF;
    for (int i = tid; i < width; i += nt) LT[i] = p.ltri[i];
    for (int i = tid; i < 2 * VIT_MAX_WAVES; i += nt) { wv[i] = NINF; wi[i] = S; }
    const int part = tid & 1;                            // which half of the band this lane scans, and which destination half it scores
    const int split = (width + 1) / 2;
    const int d0 = part * split, d1 = part ? width : split;
    const double l_same = p.l_stay, l_cross = p.l_switch;
    int b_[VIT_SLOTS]; bool act[VIT_SLOTS]; double lr[VIT_SLOTS]; float on[VIT_SLOTS];
#pragma unroll
    for (int q = 0; q < VIT_SLOTS; ++q) {
        b_[q] = (tid + q * nt) >> 1;
        act[q] = b_[q] < npb;
        lr[q] = act[q] ? p.lrow[b_[q]] : 0.0;
        on[q] = act[q] ? obs[part * npb + b_[q]] : 0.f;
    }
    auto publish = [&](int par, const Best& w) {         // the wave's best (value, first state) of the frame just written
        Best r = w;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double v = __shfl_xor(r.v, o);
            const int i = __shfl_xor(r.i, o);
            take(r, v, i);
        }
        if (lane == 0) { wv[par * VIT_MAX_WAVES + wave] = r.v; wi[par * VIT_MAX_WAVES + wave] = r.i; }
    };
    __syncthreads();                                     // the halos are in place before the first value is
    {
        Best w{NINF, S};
#pragma unroll
        for (int q = 0; q < VIT_SLOTS; ++q)
            if (act[q]) {
                const double v = log((double)on[q] + TINY_D) + (part ? p.l_init_u : p.l_tiny);
                U[part * pitch + hw + b_[q]] = v + lr[q];
                take(w, v, part * npb + b_[q]);
            }
        publish(0, w);
    }
    if (T > 1) {
#pragma unroll
        for (int q = 0; q < VIT_SLOTS; ++q) on[q] = act[q] ? obs[S + part * npb + b_[q]] : 0.f;
    }
    __syncthreads();
    for (long t = 1; t < T; ++t) {
        const int par = (int)(t & 1);
        const double* Upv = U + (par ^ 1) * 2 * pitch;   // voiced sources; the unvoiced ones follow at + pitch
        double* Uc = U + par * 2 * pitch;
        float oc[VIT_SLOTS];
#pragma unroll
        for (int q = 0; q < VIT_SLOTS; ++q) oc[q] = on[q];
        if (t + 1 < T) {                                 // the next frame's observations are under way while this one is scored
            const float* o = obs + (t + 1) * S + part * npb;
#pragma unroll
            for (int q = 0; q < VIT_SLOTS; ++q) on[q] = act[q] ? o[b_[q]] : 0.f;
        }
        Best g{NINF, S};
        {                                                // (the slots of waves that do not exist hold -inf)
            for (int k0 = 0; k0 < VIT_MAX_WAVES; k0 += 8) {
                double gv[8]; int gi[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) { gv[k] = wv[(par ^ 1) * VIT_MAX_WAVES + k0 + k]; gi[k] = wi[(par ^ 1) * VIT_MAX_WAVES + k0 + k]; }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const bool better = gv[k] > g.v || (gv[k] == g.v && gi[k] < g.i);
                    g.v = better ? gv[k] : g.v; g.i = better ? gi[k] : g.i;
                }
            }
        }
        const double fall = g.v + p.l_tiny;
        Best w{NINF, S};
#pragma unroll
        for (int q = 0; q < VIT_SLOTS; ++q) {
            if (q * nt >= S) break;                      // (uniform: no pair of this slot exists)
            const int b = act[q] ? b_[q] : 0;
            // source bin i = b - hw + dd sits at halo index b + dd; ascending source, strict >: the first maximum
            const double* sv = Upv + b;
            double mv = NINF, mu = NINF; int iv = 0, iu = 0;
            auto step = [&](int dd, double lt, double a, double c) {
                const double cv = a + lt, cu = c + lt;
                const bool gv = cv > mv, gu = cu > mu;
                mv = gv ? cv : mv; iv = gv ? dd : iv;
                mu = gu ? cu : mu; iu = gu ? dd : iu;
            };
            int dd = d0;
            for (; dd + 4 <= d1; dd += 4) {              // four cells of the band at a time: the LDS reads go out together
                double l[4], a[4], c[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { l[u] = LT[dd + u]; a[u] = sv[dd + u]; c[u] = sv[pitch + dd + u]; }
#pragma unroll
                for (int u = 0; u < 4; ++u) step(dd + u, l[u], a[u], c[u]);
            }
            for (; dd < d1; ++dd) step(dd, LT[dd], sv[dd], sv[pitch + dd]);
            // the partner lane scanned the other half of the band: the lower half comes first, so it keeps ties
            const double ov = __shfl_xor(mv, 1), ou = __shfl_xor(mu, 1);
            const int oiv = __shfl_xor(iv, 1), oiu = __shfl_xor(iu, 1);
            if (part ? !(mv > ov) : (ov > mv)) { mv = ov; iv = oiv; }
            if (part ? !(mu > ou) : (ou > mu)) { mu = ou; iu = oiu; }
            if (!act[q]) continue;
            const int kv = b - hw + iv, ku = npb + b - hw + iu;
            Best d{mv + (part ? l_cross : l_same), kv};
            take(d, mu + (part ? l_same : l_cross), ku);
            take(d, fall, g.i);
            const double nv = log((double)oc[q] + TINY_D) + d.v;
            ptr[t * S + part * npb + b] = (unsigned short)d.i;
            Uc[part * pitch + hw + b] = nv + lr[q];
            take(w, nv, part * npb + b);
        }
        publish(par, w);
        __syncthreads();
    }
    __threadfence();
    __syncthreads();
    // backtrack: the workgroup copies the back-pointers of `chunk` frames into LDS, one lane walks through them
    unsigned int* PB = (unsigned int*)(wi + 2 * VIT_MAX_WAVES);
    const unsigned short* PBs = (const unsigned short*)PB;
    int s = 0;
    if (tid == 0) {
        const int par = (int)((T - 1) & 1);
        Best g{NINF, S};
        for (int k = 0; k < nw; ++k) take(g, wv[par * VIT_MAX_WAVES + k], wi[par * VIT_MAX_WAVES + k]);
        s = min(g.i, S - 1);
        states[T - 1] = s;
    }
    for (long hi = T - 1; hi >= 1; hi -= p.chunk) {      // the rows lo + 1 .. hi
        const long lo = hi > p.chunk ? hi - p.chunk : 0;
        const int words = (int)(hi - lo) * npb;          // S is even: a row is npb 32-bit words
        const unsigned int* src = (const unsigned int*)(ptr + (lo + 1) * S);
        for (int i = tid; i < words; i += nt) PB[i] = src[i];
        __syncthreads();
        if (tid == 0)
            for (long t = hi; t > lo; --t) { s = min((int)PBs[(t - lo - 1) * S + s], S - 1); states[t - 1] = s; }
        __syncthreads();
    }
}

// tables_dev (fp64): thr[nth + 1] | beta[nth] | beta_cum[nth + 1] | bfact[n_lags + 1] | bexp[n_lags + 1] | ltri[width] | lrow[npb]
struct Tables { size_t thr, beta, beta_cum, bfact, bexp, ltri, lrow, total; };
inline Tables tables_plan(const tdx_pyin_params& q) {
    const size_t nth = (size_t)q.n_thresholds, nl = (size_t)(q.max_period - q.min_period + 1);
    Tables t{};
    size_t o = 0;
    t.thr = o; o += nth + 1;
    t.beta = o; o += nth;
    t.beta_cum = o; o += nth + 1;
    t.bfact = o; o += nl + 1;
    t.bexp = o; o += nl + 1;
    t.ltri = o; o += (size_t)q.width;
    t.lrow = o; o += (size_t)q.n_pitch_bins;
    t.total = o;
    return t;
}

int check_params(const char* fn, const tdx_pyin_params* q, bool viterbi_only) {
    const std::string at = std::string(fn) + ": ";
    if (!q) return fail(TDX_E_INVALID, at + "null argument");
    if (q->n_pitch_bins < 1 || 2 * (long)q->n_pitch_bins > MAX_STATES)
        return fail(TDX_E_INVALID, at + "2 * n_pitch_bins = " + std::to_string(2 * (long)q->n_pitch_bins) + " is outside the supported 2 .. 4096 states");
    if (q->width < 1 || q->width % 2 == 0) return fail(TDX_E_INVALID, at + "the transition width must be odd and >= 1");
    if (q->n_pitch_bins < q->width)
        return fail(TDX_E_INVALID, at + "n_pitch_bins (" + std::to_string(q->n_pitch_bins) + ") is below the transition width (" + std::to_string(q->width) + ")");
    if (q->n_thresholds < 1 || q->n_thresholds > MAX_THRESH) return fail(TDX_E_INVALID, at + "n_thresholds must lie in 1 .. 254");
    if (q->max_period - (long)q->min_period < 2 || q->min_period < 1)
        return fail(TDX_E_INVALID, at + "need min_period >= 1 and max_period - min_period >= 2");
    if (q->max_period > MAX_PERIOD) return fail(TDX_E_INVALID, at + "max_period above the supported 4096");
    if (viterbi_only) return TDX_OK;
    if (q->frame_length < 4 || q->frame_length > MAX_FRAME) return fail(TDX_E_INVALID, at + "frame_length is outside the supported 4 .. 8192");
    if (q->win_length < 1 || q->win_length >= q->frame_length) return fail(TDX_E_INVALID, at + "need 1 <= win_length < frame_length");
    if (q->hop_length < 1) return fail(TDX_E_INVALID, at + "hop_length must be >= 1");
    if (q->max_period > q->frame_length - q->win_length - 1) return fail(TDX_E_INVALID, at + "max_period exceeds frame_length - win_length - 1");
    if (!(q->sr > 0.0) || !(q->fmin > 0.0) || !(q->bins_per_octave > 0.0)) return fail(TDX_E_INVALID, at + "sr, fmin and bins_per_octave must be positive");
    return TDX_OK;
}

struct WsPlan { size_t yin, shifts, obs, ptr, total; };       // offsets in bytes
inline WsPlan ws_plan(const tdx_pyin_params& q, long frames) {
    const size_t F = (size_t)frames, nl = (size_t)(q.max_period - q.min_period + 1), S = 2 * (size_t)q.n_pitch_bins;
    auto al256 = [](size_t b) { return (b + 255) / 256 * 256; };
    WsPlan w{};
    size_t o = 0;
    w.yin = o; o += al256(F * nl * 4);
    w.shifts = o; o += al256(F * nl * 4);
    w.obs = o; o += al256(F * S * 4);
    w.ptr = o; o += al256(F * S * 2);
    w.total = o;
    return w;
}

template <typename K>
int allow_lds(K kernel, size_t bytes, const char* fn) {
    if (bytes > 160 * 1024) return fail(TDX_E_INVALID, std::string(fn) + ": the configuration needs more LDS than a workgroup has");
    if (bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return fail_hip(e, __FILE__, __LINE__);
    }
    return TDX_OK;
}

int launch_viterbi(const tdx_pyin_params& q, const double* tables, const float* obs, const long* tab, int nclips, long T1, unsigned short* ptr,
                   int* states, hipStream_t st) {
    const Tables tp = tables_plan(q);
    VitArgs va{obs, tab, T1, q.n_pitch_bins, q.width, tables + tp.ltri, tables + tp.lrow, q.log_stay, q.log_switch, q.log_init_unvoiced,
               log(TINY_D), ptr, states, vit_chunk(q.n_pitch_bins, q.width)};
    const int threads = std::min(VIT_MAX_THREADS, up(2 * q.n_pitch_bins, 64));
    const size_t lds = vit_lds_bytes(q.n_pitch_bins, q.width);
    TRY(allow_lds(pyin_viterbi_kernel, lds, "tdx_pyin_viterbi"));
    hipLaunchKernelGGL(pyin_viterbi_kernel, dim3(nclips), dim3(threads), lds, st, va);
    LAUNCH_CHECK();
    return TDX_OK;
}

}  // namespace

struct tdx_pyin {
    int device = 0;
};

extern "C" {

int tdx_pyin_create(int device, tdx_pyin** out) {
    if (!out) return tdx::fail(TDX_E_INVALID, "tdx_pyin_create: null argument");
    if (device < 0) return tdx::fail(TDX_E_INVALID, "tdx_pyin_create: device must be >= 0");
    tdx_pyin* h = new tdx_pyin();
    h->device = device;
    *out = h;
    return TDX_OK;
}

int tdx_pyin_destroy(tdx_pyin* h) {
    delete h;
    return TDX_OK;
}

size_t tdx_pyin_workspace_bytes(const tdx_pyin* h, const tdx_pyin_params* params, long total_frames) {
    if (!h || total_frames < 1 || total_frames > (1L << 31) || check_params("tdx_pyin_workspace_bytes", params, true) != TDX_OK) return 0;
    return ws_plan(*params, total_frames).total;
}

int tdx_pyin_viterbi(tdx_pyin* h, const float* obs_dev, long T, const tdx_pyin_params* params, const double* tables_dev, size_t tables_len,
                     int* states_dev, void* ws_, size_t ws_bytes, void* stream) {
    if (!h || !obs_dev || !tables_dev || !states_dev || !ws_) return tdx::fail(TDX_E_INVALID, "tdx_pyin_viterbi: null argument");
    TRY(check_params("tdx_pyin_viterbi", params, true));
    if (T < 1 || T > (1L << 31)) return tdx::fail(TDX_E_INVALID, "tdx_pyin_viterbi: T must lie in 1 .. 2^31");
    if (tables_len != tables_plan(*params).total) return tdx::fail(TDX_E_INVALID, "tdx_pyin_viterbi: tables_len does not match the parameters");
    const WsPlan wp = ws_plan(*params, T);
    if (ws_bytes < wp.total) return tdx::fail(TDX_E_WORKSPACE, "tdx_pyin_viterbi: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    return launch_viterbi(*params, tables_dev, obs_dev, nullptr, 1, T, (unsigned short*)((char*)ws_ + wp.ptr), states_dev, (hipStream_t)stream);
}

int tdx_pyin_forward(tdx_pyin* h, const float* x_dev, long n_total, const int64_t* table_host, const int64_t* table_dev, int nclips,
                     const tdx_pyin_params* params, const double* tables_dev, size_t tables_len, int* states_dev, float* voiced_prob_dev,
                     float* tap_yin_dev, float* tap_shifts_dev, float* tap_obs_dev, void* ws_, size_t ws_bytes, void* stream) {
    if (!h || !x_dev || !table_host || !table_dev || !tables_dev || !states_dev || !voiced_prob_dev || !ws_)
        return tdx::fail(TDX_E_INVALID, "tdx_pyin_forward: null argument");
    TRY(check_params("tdx_pyin_forward", params, false));
    const tdx_pyin_params& q = *params;
    if (n_total < 1) return tdx::fail(TDX_E_INVALID, "tdx_pyin_forward: n_total must be >= 1");
    if (nclips < 1 || nclips > MAX_CLIPS) return tdx::fail(TDX_E_INVALID, "tdx_pyin_forward: need 1 <= nclips <= 65535");
    if (tables_len != tables_plan(q).total) return tdx::fail(TDX_E_INVALID, "tdx_pyin_forward: tables_len does not match the parameters");
    // the table is what the kernels index with: every entry is checked here
    long frames = 0, maxT = 0;
    for (int c = 0; c < nclips; ++c) {
        const int64_t* t = table_host + (size_t)c * TAB;
        const long off = t[0], n = t[1], frame0 = t[2], T = t[3];
        const std::string at = "tdx_pyin_forward: clip " + std::to_string(c) + ": ";
        if (n < 1 || off < 0 || off > n_total || n > n_total - off) return tdx::fail(TDX_E_INVALID, at + "samples outside the input");
        if (!q.center && n < q.frame_length) return tdx::fail(TDX_E_INVALID, at + "shorter than frame_length with center off");
        const long want = q.center ? 1 + n / q.hop_length : 1 + (n - q.frame_length) / q.hop_length;
        if (T != want) return tdx::fail(TDX_E_INVALID, at + "has " + std::to_string(want) + " frames, the table says " + std::to_string(T));
        if (frame0 != frames) return tdx::fail(TDX_E_INVALID, at + "frame0 does not follow the clips before it");
        frames += T; maxT = std::max(maxT, T);
        if (frames > (1L << 31) - 1) return tdx::fail(TDX_E_INVALID, "tdx_pyin_forward: more than 2^31 - 1 frames");
    }
    const WsPlan wp = ws_plan(q, frames);
    if (ws_bytes < wp.total) return tdx::fail(TDX_E_WORKSPACE, "tdx_pyin_forward: workspace too small");
    tdx::DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return tdx::fail_hip(guard.err, __FILE__, __LINE__);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)ws_;
    float* yin = tap_yin_dev ? tap_yin_dev : (float*)(ws + wp.yin);
    float* shifts = tap_shifts_dev ? tap_shifts_dev : (float*)(ws + wp.shifts);
    float* obs = tap_obs_dev ? tap_obs_dev : (float*)(ws + wp.obs);
    const long* tab = (const long*)table_dev;
    const int n_lags = q.max_period - q.min_period + 1;
    const Tables tp = tables_plan(q);

    YinArgs ya{x_dev, tab, q.frame_length, q.win_length, q.hop_length, q.center ? q.frame_length / 2 : 0, q.min_period, q.max_period, yin, shifts};
    const int ythreads = std::min(1024, up(q.max_period, 64));
    const size_t ylds = ((size_t)q.frame_length + q.max_period + 1 + ythreads) * sizeof(float);
    TRY(allow_lds(pyin_yin_kernel, ylds, "tdx_pyin_forward"));
    hipLaunchKernelGGL(pyin_yin_kernel, dim3((unsigned)maxT, nclips), dim3(ythreads), ylds, st, ya);
    LAUNCH_CHECK();

    ObsArgs oa{yin, shifts, tab, tables_dev + tp.thr, tables_dev + tp.beta, tables_dev + tp.beta_cum, tables_dev + tp.bfact, tables_dev + tp.bexp,
               n_lags, q.n_pitch_bins, q.n_thresholds, q.min_period, q.sr, q.fmin, q.bins_per_octave, q.no_trough_prob, obs, voiced_prob_dev};
    const size_t olds = obs_lds_bytes(n_lags, q.n_pitch_bins, q.n_thresholds);
    TRY(allow_lds(pyin_obs_kernel, olds, "tdx_pyin_forward"));
    hipLaunchKernelGGL(pyin_obs_kernel, dim3((unsigned)maxT, nclips), dim3(OBS_THREADS), olds, st, oa);
    LAUNCH_CHECK();

    return launch_viterbi(q, tables_dev, obs, tab, nclips, 0, (unsigned short*)(ws + wp.ptr), states_dev, st);
}

}  // extern "C"
