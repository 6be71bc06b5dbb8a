// spk_k_iter.hip -- the fused iteration kernels on the un-normalised basis: kernel B (MAXPY + norm + next PCApply) of
// forms 5 and 7, and form 7's single launch of VecMDot and kernel B.
#include "spk_device.hpp"

namespace spk {
namespace k {

// ---------------------------------------------------------------------------
// Kernel B (opts.iteration_form = 5; the second half of form 7).  One iteration of form 5 is three launches: VecMDot (RAW
// inner products of the un-normalised basis V~_i with w~, and B D w~), kernel B, and the plain product K z~, whose rider
// workgroup runs the Givens step and the new scale factor (GivensRider).  No vector is normalised in memory: V~_i carries
// one scale factor sc_i = 1 / ||w'_i||, applied to the reduced scalars (h_i = sc_i s_w (V~_i . w~), ...).
//
//   B  iter_maxpy_uhead_kernel w' = s_w w~ - sum_i (h_i sc_i) V~_i (VecMAXPY) with ||w'||^2 from the same pass (VecNorm),
//                              and the next iteration's preconditioner and B^T product applied to the UN-normalised w'
//                              (both are linear): z~ = D w' - (B D)^T y~, c~ = B^T y~.  y~ needs t~ = B D w', a reduction
//                              over the very vector this pass builds; it follows from q by linearity,
//                              t~ = q - sum_i h_i (B D v_i) -- an identity between sums of the same magnitude (no squares:
//                              none of the Pythagorean norm's cancellation), kept per basis vector in tb[].
//
// The scalar workgroup streams nothing in kernel B: it writes the multiplier entries and reduces ||w'||^2 (with defer_fin
// it leaves the partials to the rider of the next product launch).
// ---------------------------------------------------------------------------
// The body of kernel B (iter_maxpy_uhead_kernel, gs_fused_kernel).  scalar_wg: the workgroup that also writes the
// multiplier entries of w', z~, c~, tb, the Hessenberg column and the multiplier entries' share of ||w'||^2 (a workgroup
// of its own in kernel B, one of the streaming ones in the fused launch); dots(i, j, a, c): the reduced [h, q] values i
// and j into a and c (an index < 0: none, the value stays) -- in form 7 a wait, so both are requested before either is
// looked at and every load that does not depend on them is requested first.
// keep (form 7 only, see KeepSet): the first tile takes w~, the parity planes and V_0 .. V_{KV-1} from the keep set; its
// loads ahead of the scalar prologue are D^-1, the first group behind the kept vectors and Keep::AH vectors of the group
// behind that one (held in the tile loop's buffer).  Groups, slots past nv and the order of every addition are those of
// the other tiles.
// BT = float (-spk_basis_precision single, b.w32): V~_0 .. V~_{nv-1} are read as floats (converted exactly), w' is formed in
// FP64 as ever and stored as float(w') into w32, ||w'||^2 is the norm of the ROUNDED vector -- so that the scale factor
// belongs to what the basis holds -- and z~, c~ come from the unrounded w' in registers (the method is flexible).
template <int T, int G, int U, int MP, class Dots, class Keep = NoKeep, class BT = double>
__device__ __forceinline__ void maxpy_uhead_tiles(const IterB &b, int scalar_wg, Dots dots, Keep *keep = nullptr)
{
    constexpr bool F32 = std::is_same<BT, float>::value;
    static_assert(!F32 || !Keep::any, "the keep set holds FP64 operands");
    using Basis = BasisElem<BT>;
    using E2 = typename Basis::E2;
    constexpr int KW = Keep::KW, KP = Keep::KP, KV = Keep::KV;
    static_assert(KV % G == 0, "whole groups of basis vectors are kept");
    // the kept tile: AH more vectors requested ahead of the totals wait, into the tile loop's buffer (see NoKeep)
    constexpr int AH = Keep::AH;
    static_assert(AH <= G, "the tile loop's buffer is one group");
    const int32_t dn = __builtin_nontemporal_load(b.done);  // looked at behind the first loads (see mdot_ws16_kernel)
    __shared__ double hs[kMaxNv], lam[kMaxNv * 8], ys[8], wraws[8], tus[8];
    __shared__ double red[T];
    const int nv = b.nv, m = b.m;
    constexpr int NP = MP > 0 ? MP : 1;
    const int gmain = b.gmain;
    const bool is_main = (int)blockIdx.x < gmain;
    const int64_t n2 = b.nl / 2;
    const int bid = blockIdx.x;
    // with a halo to send the grid is walked from both ends inwards (the rows the neighbours wait for leave first)
    const int bx = b.sr.peer ? ((bid & 1) ? gmain - 1 - (bid >> 1) : (bid >> 1)) : bid;

    // ---- a streaming workgroup puts the loads of its first tile in flight BEFORE the scalar prologue: w, D, the
    // planes of B D and the first group of basis vectors depend on none of it, and the prologue is a chain of two
    // memory round trips of its own (kernel of 16 us on the 1/8 slab, 8 us of them not bytes)
    constexpr bool PRE = U * (MP > 0 ? MP : 1) <= 16;  // planes of B D fetched ahead too, where the registers allow (not 512 x 4 x 8 rows)
    static_assert(KP == 0 || (PRE && KP <= NP / 2), "kept planes are parity planes fetched ahead");
    // Keep::PK: the launcher vouches for parity planes (b.packed), so only NP / 2 planes are fetched ahead -- the registers
    // of the other half hold the loads requested ahead of the totals wait instead
    constexpr bool PK = Keep::PK;
    constexpr int NPE = PK ? NP / 2 : NP;
    static_assert(!PK || (PRE && MP > 0), "parity planes fetched ahead");
    const bool packed = PK || b.packed;
    const bool kpl = KP > 0 && packed && m > 0;   // (as in mdot_tiles: the first tile's planes are in the keep set)
    double2 wv[U], dv[U], pe[PRE ? NPE : 1][U], tdead;
    E2 t0[G][U], t[G][U];   // t: the tile loop's buffer (empty until the loop's first trip past t0)
    int64_t idx[U];
    bool ok[U];
    int64_t tile = bx;
    auto load_planes = [&]() {
#pragma unroll
        for (int q = 0; q < NPE; ++q) {
            const bool live = packed ? 2 * q < m : q < m;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                pe[q][u].x = pe[q][u].y = 0.0;
                if (live) pe[q][u] = ld2s<true>(b.bd + (size_t)q * b.ldb, idx[u]);
            }
        }
    };
    auto load_tile = [&](int64_t tl, bool KF) {   // KF: the kept tile
#pragma unroll
        for (int u = 0; u < U; ++u) {
            idx[u] = tl * (T * U) + u * T + threadIdx.x;
            ok[u] = idx[u] < n2;
            if (!ok[u]) idx[u] = 0;
            wv[u] = KF && KW ? keep->get(0, u) : ld2(b.w, idx[u]);
            dv[u] = ld2(b.dinv, idx[u]);
        }
        if (MP > 0 && PRE) {
            if (KF && kpl) {
#pragma unroll
                for (int q = 0; q < NPE; ++q) {
#pragma unroll
                    for (int u = 0; u < U; ++u) pe[q][u] = q < KP ? keep->get(KW + q, u) : double2{0.0, 0.0};
                }
            } else {
                load_planes();
            }
        }
        if (KF && KV > 0) tdead = ld2s<true>(b.V, 0);   // what a slot past nv loads
        const int v0 = KF ? KV : 0;   // the first group that is not kept
#pragma unroll
        for (int v = 0; v < G; ++v) {
            const bool live = v0 + v < nv;
#pragma unroll
            for (int u = 0; u < U; ++u) t0[v][u] = Basis::ld(b.V, (size_t)(live ? v0 + v : 0), b.ldv, live ? idx[u] : 0);
        }
        if (KF && AH > 0) {   // ... and of the group behind it: the first trip of the tile loop finds them here
#pragma unroll
            for (int v = 0; v < AH; ++v) {
                const bool live = v0 + G + v < nv;
#pragma unroll
                for (int u = 0; u < U; ++u) t[v][u] = Basis::ld(b.V, (size_t)(live ? v0 + G + v : 0), b.ldv, live ? idx[u] : 0);
            }
        }
    };
    bool have = is_main && tile * (T * U) < n2;
    if (have) load_tile(tile, Keep::any);

    // ---- scalars, derived by every workgroup from the reduced [h, q]; all their loads first
    double lamv = 0.0;
    const bool lam_mine = (int)threadIdx.x < nv * m;
    if (lam_mine) lamv = Basis::at(b.V, (size_t)(threadIdx.x / m), b.ldv, b.nl + (threadIdx.x % m));
    double wl = 0.0, sh = 1.0;
    if ((int)threadIdx.x < m) {
        wl = b.wl_in[threadIdx.x];
        sh = b.shat[threadIdx.x];
    }
    double hi_pre = 0.0, qv_pre = 0.0, tbv_pre[8], sci = 1.0;
    const double s_w = b.sc[nv - 1];   // w = s_w w~
    if (threadIdx.x < kWave) {
        const int i = threadIdx.x;
        sci = i < nv ? b.sc[i] : 0.0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            // an FP32 basis: B D of the newest vector AS STORED comes from MDot (behind w.w), not from the recurrence value
            // the previous kernel B left for the unrounded w'
            if (F32 && i == nv - 1) tbv_pre[r] = r < m ? b.dots[nv + m + 1 + r] : 0.0;
            else tbv_pre[r] = (r < m && i < nv) ? b.tb[i * 8 + r] : 0.0;
        }
        dots(i < nv ? i : -1, i < m ? nv + i : -1, hi_pre, qv_pre);
    }
    if (dn) return;
    if (Keep::fused) GS_STAMP(kGsTotalsSeen);
    if (threadIdx.x < kWave) {  // lane i owns basis vector i (nv <= 63)
        const int i = threadIdx.x;
        // un-normalised basis: h_i = sc_i s_w (V~_i . w~); the MAXPY coefficient of V~_i and the weight of B D V~_i is h_i sc_i
        const double hi = sci * s_w * hi_pre;
        const double ci = hi * sci;
        double tbv[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) tbv[r] = tbv_pre[r] * sci;
        const double qv = qv_pre * s_w;
        if (i < nv) hs[i] = ci;
        if ((int)blockIdx.x == scalar_wg && i < nv) b.hbuf[i] = hi;  // the Hessenberg column (reducer only)
        if (F32 && (int)blockIdx.x == scalar_wg && i == nv - 1) {   // ... and kept for the iterations to come
#pragma unroll
            for (int r = 0; r < 8; ++r)
                if (r < m) b.tb[(size_t)i * 8 + r] = tbv_pre[r];
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if (r < m) {  // uniform
                const double tsum = wave_sum(hi * tbv[r]);
                const double qr = __shfl(qv, r, kWave);
                if (i == 0) tus[r] = qr - tsum;  // B D w' = B D w - sum h_i (B D v_i)
            }
        }
    }
    if (lam_mine) lam[threadIdx.x] = lamv;
    for (int t = threadIdx.x + T; t < nv * m; t += T) lam[t] = Basis::at(b.V, (size_t)(t / m), b.ldv, b.nl + (t % m));
    __syncthreads();
    if ((int)threadIdx.x < NP && MP > 0) {
        const int r = threadIdx.x;
        double y = 0.0, wraw = 0.0;
        if (r < m) {
            wraw = s_w * wl;
            for (int i = 0; i < nv; ++i) wraw += -hs[i] * lam[i * m + r];  // the MAXPY of the multiplier entries
            y = -(wraw - tus[r]) / sh;
        }
        wraws[r] = wraw;
        ys[r] = y;
    }
    __syncthreads();
    double yv[NP];
#pragma unroll
    for (int r = 0; r < NP; ++r) yv[r] = MP > 0 ? ys[r] : 0.0;
    if (Keep::fused) GS_STAMP(kGsPrologueDone);
    if (have) {  // w = s_w w~
#pragma unroll
        for (int u = 0; u < U; ++u) {
            wv[u].x *= s_w;
            wv[u].y *= s_w;
        }
    }

    if ((int)blockIdx.x == scalar_wg) {
        // ---- the scalar / reducing workgroup: multiplier entries of w', z~, c~; B D w' for the recurrence
        if ((int)threadIdx.x < m) {
            const int r = threadIdx.x;
            double w1 = tus[r];
            if (b.fact == SPK_SCHUR_FULL)
                for (int q = 0; q < m; ++q) w1 -= b.gram[r * m + q] * ys[q];
            if (!b.dead_out) {
                if (F32) b.w32[b.nl + r] = (float)wraws[r];
                else b.w[b.nl + r] = wraws[r];
                b.zun[b.nl + r] = ys[r];
                b.c[b.nl + r] = w1;
            }
            b.tb[(size_t)nv * 8 + r] = tus[r];  // un-normalised: scaled by sc where it is read
            b.wl_out[r] = w1;
        }
        __syncthreads();
        double lam2 = 0.0;  // the multiplier entries' share of ||w'||^2 (rank 0 only)
        if (threadIdx.x == 0)
            for (int r = 0; r < m; ++r) {
                const double wr = F32 ? (double)(float)wraws[r] : wraws[r];   // (the norm of what the basis holds)
                lam2 += b.lam_in_dot ? wr * wr : 0.0;
            }
        if (b.defer_fin) {
            // un-normalised basis: nothing in the product launch that follows needs ||w'||^2 except its rider workgroup
            // (scale factor, Givens step), so the rider also REDUCES the partials (and all-reduces the sum) beside the
            // row tiles: this launch ends with its last streaming workgroup -- no publish -> re-read tail
            if (threadIdx.x == 0) publish(b.partials + (size_t)gmain * kPartialLd, lam2);
            if (!is_main) return;   // (the fused launch: this workgroup streams its tiles too)
        } else if (Keep::fused) {
            // the fused launch behind the cycle's last iteration: this workgroup streams its tiles first and reduces the
            // norm behind them, below (lam is dead behind the prologue: it carries the multiplier entries' share there)
            if (threadIdx.x == 0) lam[0] = lam2;
        } else {
            final_reduce(b.partials, gmain, kPartialLd, 1, red, FinErr{b.err, b.fin_ticks});
            if (threadIdx.x == 0) red[0] = red[0] + lam2;
            __syncthreads();
            if (b.ar.P) peer_allreduce_block(b.ar, red, 1, b.out);
            else if (threadIdx.x == 0) b.out[0] = red[0];
            return;
        }
    }
    if (!is_main) {  // peer-store halo: unpack this rank's ghost rows (see fused_head_kernel)
        const int64_t g = (int64_t)((int)blockIdx.x - gmain) * T + threadIdx.x;
        if (g < 2 * (int64_t)b.sr.nrecv) {
            uint32_t lo;
            const unsigned long long tw0 = (b.sr.stats && threadIdx.x == 0) ? wall_clock64() : 0ull;
            const bool okw = granule_wait(b.sr.mine + g, b.sr.seq, b.sr.timeout_ms, lo, b.sr.err, b.done);
            if (b.sr.stats && threadIdx.x == 0) {
                atomicAdd(b.sr.stats + 2 * kStatHalo, wall_clock64() - tw0);
                atomicAdd(b.sr.stats + 2 * kStatHalo + 1, 1ull);
            }
            const uint32_t other = __shfl_xor(lo, 1, kWave);
            if (!(g & 1)) b.sr.xghost[g >> 1] = join_halves(lo, other);
            if (!okw) raise_comm_error(b.sr.err, 18, b.sr.seq);
        }
        return;
    }
    double nrm = 0.0;
    bool KF = Keep::any;   // the tile at hand is the first one: its kept basis vectors come out of the keep set
    while (have) {
        const int v0 = KF ? KV : 0;
        double2 sv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) sv[u].x = sv[u].y = 0.0;
        if (MP > 0 && !PRE) {  // fat workgroups with many rows: one plane at a time
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const bool live = b.packed ? 2 * q < m : q < m;
                if (live) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const double2 e = ld2s<true>(b.bd + (size_t)q * b.ldb, idx[u]);
                        if (b.packed) {
                            sv[u].x += e.x * yv[2 * q];
                            sv[u].y += e.y * yv[2 * q + 1];
                        } else {
                            sv[u].x += e.x * yv[q];
                            sv[u].y += e.y * yv[q];
                        }
                    }
                }
            }
        } else if (MP > 0) {
            if (packed) {
#pragma unroll
                for (int q = 0; q < NP / 2; ++q) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        sv[u].x += pe[q][u].x * yv[2 * q];
                        sv[u].y += pe[q][u].y * yv[2 * q + 1];
                    }
                }
            } else if constexpr (!PK) {
#pragma unroll
                for (int r = 0; r < NP; ++r) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        sv[u].x += pe[r][u].x * yv[r];
                        sv[u].y += pe[r][u].y * yv[r];
                    }
                }
            }
        }
        // kept basis vectors, in the groups of the other tiles (a group past the first runs only below nv)
#pragma unroll
        for (int s = 0; s < KV; ++s) {
            if (KF && (s < G || s / G * G < nv)) {  // wave-uniform
                const bool live = s < nv;
                const double ai = live ? -hs[s] : 0.0;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    double2 tk = tdead;
                    if (live) tk = keep->get(KW + KP + s, u);
                    wv[u].x += ai * tk.x;
                    wv[u].y += ai * tk.y;
                }
            }
        }
        // first group of basis vectors that is not kept: already here
        if (v0 == 0 || v0 < nv) {
#pragma unroll
            for (int v = 0; v < G; ++v) {
                const double ai = v0 + v < nv ? -hs[v0 + v] : 0.0;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    wv[u].x += ai * (double)t0[v][u].x;
                    wv[u].y += ai * (double)t0[v][u].y;
                }
            }
        }
        for (int g0 = v0 + G; g0 < nv; g0 += G) {
            const bool first = AH > 0 && KF && g0 == v0 + G;   // its first AH vectors: requested ahead of the totals wait (load_tile)
            double ai[G];
#pragma unroll
            for (int v = 0; v < G; ++v) {
                const bool live = g0 + v < nv;
                const int ic = live ? g0 + v : 0;
                const bool pre = first && v < AH;
                ai[v] = live ? -hs[ic] : 0.0;
                if (!pre) {
#pragma unroll
                    for (int u = 0; u < U; ++u) t[v][u] = Basis::ld(b.V, (size_t)ic, b.ldv, live ? idx[u] : 0);
                }
            }
#pragma unroll
            for (int v = 0; v < G; ++v) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    wv[u].x += ai[v] * (double)t[v][u].x;
                    wv[u].y += ai[v] * (double)t[v][u].y;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (ok[u]) {
                const int64_t i = idx[u];
                double2 zz, cc;
                float2 wf;
                if (F32) {
                    wf.x = (float)wv[u].x;   // round to nearest
                    wf.y = (float)wv[u].y;
                    nrm += (double)wf.x * (double)wf.x;
                    nrm += (double)wf.y * (double)wf.y;
                } else {
                    nrm += wv[u].x * wv[u].x;
                    nrm += wv[u].y * wv[u].y;
                }
                zz.x = wv[u].x * dv[u].x;
                zz.y = wv[u].y * dv[u].y;
                if (MP > 0 && b.fact == SPK_SCHUR_FULL) {
                    zz.x -= sv[u].x;
                    zz.y -= sv[u].y;
                }
                // streamed out past the L2 (non-temporal stores): nobody on this XCD reads them again before the kernel
                // boundary writes them back anyway (same box, alternating: 512^2 60.6 -> 59.1 us per iteration, 1024^2 203.3 -> 202.1, 1/8 slab 39.3 -> 39.0)
                if (!b.dead_out) {
                    if (F32) stf2nt(b.w32, i, wf);
                    else st2nt(b.w, i, wv[u]);
                    st2nt(b.zun, i, zz);
                    if (MP > 0) {
                        cc.x = sv[u].x / dv[u].x;
                        cc.y = sv[u].y / dv[u].y;
                        st2nt(b.c, i, cc);
                    }
                }
                for (int q = 0; q < b.sr.n; ++q) {
                    const int64_t e = 2 * i - b.sr.r0[q];
                    if (b.sr.peer) {
                        const unsigned long long tag = (unsigned long long)b.sr.seq << 32;
                        if (e >= 0 && e < b.sr.len[q]) {
                            const unsigned long long bits = (unsigned long long)__double_as_longlong(zz.x);
                            st_sys(b.sr.remote[q] + 2 * e, tag | (bits & 0xffffffffull));
                            st_sys(b.sr.remote[q] + 2 * e + 1, tag | (bits >> 32));
                        }
                        if (e + 1 >= 0 && e + 1 < b.sr.len[q]) {
                            const unsigned long long bits = (unsigned long long)__double_as_longlong(zz.y);
                            st_sys(b.sr.remote[q] + 2 * e + 2, tag | (bits & 0xffffffffull));
                            st_sys(b.sr.remote[q] + 2 * e + 3, tag | (bits >> 32));
                        }
                    } else {
                        if (e >= 0 && e < b.sr.len[q]) b.sr.buf[b.sr.off[q] + e] = zz.x;
                        if (e + 1 >= 0 && e + 1 < b.sr.len[q]) b.sr.buf[b.sr.off[q] + e + 1] = zz.y;
                    }
                }
            }
        }
        tile += gmain;
        have = tile * (T * U) < n2;
        if (have) {
            load_tile(tile, false);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                wv[u].x *= s_w;
                wv[u].y *= s_w;
            }
        }
        KF = false;
    }
    // ||w'||^2 of this workgroup's entries.  The partial goes to slot bx -- the FIRST TILE this workgroup
    // streamed -- so that the reducer adds the partials in tile order whichever way the grid was walked
    // (bit-identical norms with and without the peer-store halo in the same launch)
    if (Keep::fused) GS_STAMP(kGsBTilesDone);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double sw = wave_sum(nrm);
    if (lane == 0) red[wave] = sw;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tsum = 0.0;
#pragma unroll
        for (int j = 0; j < T / kWave; ++j) tsum += red[j];
        publish(b.partials + (size_t)bx * kPartialLd, tsum);
    }
    if (Keep::fused && (int)blockIdx.x == scalar_wg && !b.defer_fin) {
        // no product follows the cycle's last iteration, so no rider reduces the norm: kernel B's own order (the partials
        // in tile order, then the multiplier entries' share), here behind this workgroup's tiles
        __syncthreads();
        final_reduce(b.partials, gmain, kPartialLd, 1, red, FinErr{b.err, b.fin_ticks});
        if (threadIdx.x == 0) b.out[0] = red[0] + lam[0];
    }
}
template <int T, int G, int U, int MP, class BT = double>
__global__ __launch_bounds__(T) void iter_maxpy_uhead_kernel(IterB b)
{
    const int nhalo = b.sr.peer ? (2 * b.sr.nrecv + T - 1) / T : 0;
    auto dots = [&](int i, int j, double &a, double &c) {
        if (i >= 0) a = b.dots[i];
        if (j >= 0) c = b.dots[j];
    };
    maxpy_uhead_tiles<T, G, U, MP, decltype(dots), NoKeep, BT>(b, b.gmain + nhalo, dots);
}

int iter_maxpy_uhead(IterB b, hipStream_t s)   // returns the number of partial rows its norm is spread over (defer_fin)
{
    const int64_t n2 = b.nl / 2;
    // thin workgroups below 0.5 M entries (as MAXPY), fat ones above
    const bool thin = n2 < (int64_t)kVecMaxBlocks * 2048;
    static const int t128 = [] { const char *e = getenv("SPK_B_T128"); return e ? atoi(e) : 0; }();
    const int U = thin ? (n2 < (int64_t)kVecMaxBlocks * 1024 ? 1 : 2) : 4;
    // the smallest vectors (<= 1024 tiles of 128 double2): two-wave workgroups, twice the waves in flight per CU
    const bool tiny = thin && U == 1 && t128 && n2 <= (int64_t)1024 * 128;
    const int T = tiny ? 128 : (thin ? 256 : 512);
    int64_t tiles = (n2 + (int64_t)T * U - 1) / ((int64_t)T * U);
    if (tiles < 1) tiles = 1;
    b.gmain = (int)std::min<int64_t>(tiles, thin ? 1024 : kVecMaxBlocks);
    int grid = b.gmain + 1;
    if (b.sr.peer) grid += (2 * b.sr.nrecv + T - 1) / T;
    if (b.nv + b.m > kMaxNv - 1) fail(SPK_ERR_ARG, "iter_maxpy_uhead: %d values exceed one reduction", b.nv + b.m);
#define SPK_IB(TT, GG, UU, MPP) hipLaunchKernelGGL((iter_maxpy_uhead_kernel<TT, GG, UU, MPP>), dim3(grid), dim3(TT), 0, s, b)
    const int mp = plane_class(b.m);
    if (b.w32) {
        // an FP32 basis: the same thread positions, so a basis load is 8 bytes per lane -- twice the vectors are loaded
        // together instead (the same bytes in flight, the same registers as the FP64 groups)
        if (b.sr.n || b.sr.peer || b.ar.P) fail(SPK_ERR_STATE, "iter_maxpy_uhead: an FP32 basis runs on one rank");
#define SPK_IBF(TT, GG, UU, MPP) hipLaunchKernelGGL((iter_maxpy_uhead_kernel<TT, GG, UU, MPP, float>), dim3(grid), dim3(TT), 0, s, b)
#define SPK_IBF_MP(MPP)                                     \
    do {                                                    \
        if (!thin) SPK_IBF(512, 8, 4, MPP);                 \
        else if (U == 2) SPK_IBF(256, 16, 2, MPP);          \
        else SPK_IBF(256, 16, 1, MPP);                      \
    } while (0)
        if (mp == 0) SPK_IBF_MP(0);
        else if (mp == 4) SPK_IBF_MP(4);
        else SPK_IBF_MP(8);
#undef SPK_IBF_MP
#undef SPK_IBF
        return b.gmain;
    }
    static const int deep = [] { const char *e = getenv("SPK_VEC_DEEP"); return e ? atoi(e) : 0; }();
    // thin forms: the whole basis in one group of loads where registers allow (see maxpy)
    const int g1 = !deep || b.nv <= 8 ? 8 : (b.nv <= 16 ? 16 : 32), g2 = !deep || b.nv <= 8 ? 8 : 16;
#define SPK_IB_MP(MPP)                                                           \
    do {                                                                         \
        if (!thin) SPK_IB(512, 4, 4, MPP);                                       \
        else if (tiny) SPK_IB(128, 8, 1, MPP);                                   \
        else if (U == 2) { if (g2 == 16) SPK_IB(256, 16, 2, MPP); else SPK_IB(256, 8, 2, MPP); } \
        else if (g1 == 32) SPK_IB(256, 32, 1, MPP);                              \
        else if (g1 == 16) SPK_IB(256, 16, 1, MPP);                              \
        else SPK_IB(256, 8, 1, MPP);                                             \
    } while (0)
    if (mp == 0) SPK_IB_MP(0);
    else if (mp == 4) SPK_IB_MP(4);
    else SPK_IB_MP(8);
#undef SPK_IB_MP
#undef SPK_IB
    return b.gmain;
}

// ---------------------------------------------------------------------------
// Form 7 (opts.iteration_form = 7; what AUTO takes on one rank with fat vectors): VecMDot and kernel B in ONE launch.
// Kernel B needs ~40 reduced scalars from MDot; everything else it reads (basis rows, w~, D^-1, the planes of B D) is known
// when MDot starts.  On the 256 x 512-thread grid of the fat vector shape every workgroup
//   1. runs exactly mdot_kernel's tiles and publishes its partials (columns 1.. of the partial rows: column 0 carries the
//      ||w'||^2 partials of step 3, which the rider of the next product launch reduces);
//   2. the last workgroup reduces them as mdot_kernel does and publishes the totals, write-through, into a line armed
//      with the sentinel (a value is its own flag; the launch arms the OTHER of two lines for the next launch);
//   3. every workgroup requests its first tile of kernel B, then waits for the totals it needs, and runs kernel B's body;
//      kernel B's scalar workgroup duties go to workgroup grid - 2 (one that streams the fewest MDot tiles).
// The operands of a workgroup's first tile, the same tile in both passes, stay on chip between them (GsKeep below).
// The tile mapping and every summation order are those of the two launches: the results are the same bits.  The waits
// need every workgroup resident at once (gs_fused_occupancy) and are bounded: a wait that gives up raises the context's
// execution-error word.
// ---------------------------------------------------------------------------
struct TotalsWait {   // kernel B's dots: spins (bounded) while a value it needs still is the sentinel of the totals line
    const double *tot;
    FinErr fe;
    __device__ void operator()(int i, int j, double &a, double &c) const
    {
        // both values are requested together: one round trip behind the reducer's publish, not one per value
        double v = i >= 0 ? peek(tot + i) : 0.0, q = j >= 0 ? peek(tot + j) : 0.0;
        if (is_sentinel(v) || is_sentinel(q)) {
            const unsigned long long t0 = wall_clock64();
            do {
                __builtin_amdgcn_s_sleep(1);
                if (i >= 0) v = peek(tot + i);
                if (j >= 0) q = peek(tot + j);
            } while ((is_sentinel(v) || is_sentinel(q)) && wall_clock64() - t0 < (unsigned long long)fe.ticks &&
                     !(fe.err && __hip_atomic_load(fe.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
            if ((is_sentinel(v) || is_sentinel(q)) && fe.err) __hip_atomic_store(fe.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (i >= 0) a = v;
        if (j >= 0) c = q;
    }
};

// The keep set of instantiation <NG, MP> (GsKnobs::keep; without it an empty one): w~ and, where kernel B fetches them
// ahead (MP = 4), the two parity planes in registers, V_0 .. V_3 in LDS (4 x 32 KiB beside 12 992 B; a fifth does not
// fit 160 KiB).  Sized by the compiler's resource remark on gfx950 (tests/test_gs_resources_cpu.py):
// no scratch, <= 256 registers for every instantiation -- <5, 4> with the planes kept spills 19 VGPRs, so it keeps
// w~ and the basis vectors only.
template <int NG, int MP, int AH = 0>
struct GsKeep {
    static constexpr int KP = MP == 4 && NG <= 4 ? 2 : 0, KV = 4;
    using type = KeepSet<kGsT, kGsU, 1, KP, KV, 1 + KP, AH, (MP == 4 && AH > 0)>;
};

template <int NG, int MP, bool KEEP, int AH = 0>
__global__ __launch_bounds__(kGsT) void gs_fused_kernel(IterB b, GsArgs g)
{
    constexpr int NA = NG * 8 + 1, W = kGsT / kWave;
    static_assert(KEEP || AH == 0, "loads ahead of the wait belong to the launch with a keep set");
    using Keep = typename std::conditional<KEEP, typename GsKeep<NG, MP, AH>::type, KeepSet<kGsT, kGsU, 0, 0, 0, 0>>::type;
    __shared__ double lds[(W * NA > kGsT) ? W * NA : kGsT];
    __shared__ double2 klds[Keep::KL > 0 ? Keep::KL * kGsU * kGsT : 1];
    Keep keep;
    keep.l = klds;
    GS_STAMP(kGsEntryRaw);
    if (blockIdx.x == 0 && threadIdx.x < kWave) publish(g.tot_next + threadIdx.x, __longlong_as_double((long long)kSentinelBits));
    // the gate is requested here and looked at behind the first tile's first loads (as kernel B's body does): a gated
    // launch still ends after one round trip, with nothing published and the armed totals line untouched
    const int32_t dn = __builtin_nontemporal_load(b.done);
    if (mdot_tiles<NG, kGsT, kGsG, true, kGsU, Keep, true>(b.V, b.ldv, g.cnt, g.V2, b.nv, b.w, g.n2, g.n_dot, g.partials, 1, g.split,
                                                           lds, &keep, dn))
        return;
    if (arrive_last(gridDim.x)) {
        const int k = g.cnt + 1;
        final_reduce(g.partials, gridDim.x, kPartialLd, k, lds, g.fe);
        if ((int)threadIdx.x < k) {
            g.out[threadIdx.x] = lds[threadIdx.x];
            publish(g.tot + threadIdx.x, lds[threadIdx.x]);
        }
    }
    maxpy_uhead_tiles<kGsT, kGsG, kGsU, MP>(b, (int)gridDim.x - 2, TotalsWait{g.tot, g.fe}, &keep);
}

// The default launch -- gs_fused_kernel<NG, MP, true, AH> line by line -- with a short remainder tile staged in LDS
// (SPK_GS_TAIL, kGsKeepAheadTail): the remainder behind the whole tiles, at 1024^2 with the full Schur preconditioner two
// double2 (the multiplier entries), is requested at entry by the workgroup the tile loop would give it to and added
// behind that workgroup's loop (mdot_tiles, TAIL), instead of costing it a trip of dependent loads while every other
// workgroup has finished its tiles and waits for the totals.  A kernel of its own, not one more template argument: the
// instantiations above keep their names and, to the instruction, their code.
template <int NG, int MP, int AH>
__global__ __launch_bounds__(kGsT) void gs_fused_tail_kernel(IterB b, GsArgs g)
{
    constexpr int NA = NG * 8 + 1, W = kGsT / kWave;
    using Keep = typename GsKeep<NG, MP, AH>::type;
    __shared__ double lds[(W * NA > kGsT) ? W * NA : kGsT];
    __shared__ double2 klds[Keep::KL * kGsU * kGsT];
    __shared__ double2 tlds[kGsTailSrc * kGsTailMax];
    Keep keep;
    keep.l = klds;
    GS_STAMP(kGsEntryRaw);
    if (blockIdx.x == 0 && threadIdx.x < kWave) publish(g.tot_next + threadIdx.x, __longlong_as_double((long long)kSentinelBits));
    const int32_t dn = __builtin_nontemporal_load(b.done);   // a gated launch returns before anything is staged
    if (mdot_tiles<NG, kGsT, kGsG, true, kGsU, Keep, true, true>(b.V, b.ldv, g.cnt, g.V2, b.nv, b.w, g.n2, g.n_dot, g.partials, 1,
                                                                 g.split, lds, &keep, dn, tlds))
        return;
    if (arrive_last(gridDim.x)) {
        const int k = g.cnt + 1;
        final_reduce(g.partials, gridDim.x, kPartialLd, k, lds, g.fe);
        if ((int)threadIdx.x < k) {
            g.out[threadIdx.x] = lds[threadIdx.x];
            publish(g.tot + threadIdx.x, lds[threadIdx.x]);
        }
    }
    maxpy_uhead_tiles<kGsT, kGsG, kGsU, MP>(b, (int)gridDim.x - 2, TotalsWait{g.tot, g.fe}, &keep);
}

// f(NG, MP) as std::integral_constant values, for the fifteen <NG, MP> the fused kernels are built for
template <int N> using GsInt = std::integral_constant<int, N>;
template <class F>
inline void gs_dispatch(int ng, int mp, F &&f)
{
    if (ng < 1 || ng > 5 || (mp != 0 && mp != 4 && mp != 8))
        fail(SPK_ERR_ARG, "gs_fused: no kernel for %d groups of dot products and plane class %d", ng, mp);
    const auto groups = [&](auto mpc) {
        ng == 1 ? f(GsInt<1>{}, mpc) : ng == 2 ? f(GsInt<2>{}, mpc) : ng == 3 ? f(GsInt<3>{}, mpc)
                                     : ng == 4 ? f(GsInt<4>{}, mpc) : f(GsInt<5>{}, mpc);
    };
    mp == 0 ? groups(GsInt<0>{}) : mp == 4 ? groups(GsInt<4>{}) : groups(GsInt<8>{});
}
// the kernel of variant v at <NG, MP>
template <int NG, int MP>
inline auto gs_kernel(GsVariant v) -> void (*)(IterB, GsArgs)
{
    constexpr int AH = kGsAhead[MP / 4][NG - 1];
    switch (v) {
    case kGsKeep: return gs_fused_kernel<NG, MP, true>;
    case kGsKeepAhead: return gs_fused_kernel<NG, MP, true, AH>;
    case kGsKeepAheadTail: return gs_fused_tail_kernel<NG, MP, AH>;
    case kGsPlain: return gs_fused_kernel<NG, MP, false>;
    }
    fail(SPK_ERR_ARG, "gs_fused: unknown variant %d", (int)v);
}

int gs_fused_occupancy(int ng, int m, bool keep)
{
    // with a keep set: the fewest of the three variants SPK_GS_AHEAD and SPK_GS_TAIL choose between
    int nb = 1 << 30;
    gs_dispatch(ng, plane_class(m), [&](auto ngc, auto mpc) {
        for (int v = keep ? kGsKeep : kGsPlain; v <= (keep ? kGsKeepAheadTail : kGsPlain); ++v) {
            int n = 0;
            SPK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, gs_kernel<ngc.value, mpc.value>((GsVariant)v), kGsT, 0));
            nb = std::min(nb, n);
        }
    });
    return nb;
}

int gs_fused(IterB b, GsArgs g, GsVariant v, hipStream_t s)
{
    const int64_t grid = gs_fused_grid(b.nl);
    const VecShape vs = vec_shape(g.n2);
    if (!grid || vs.T != kGsT || vs.U != kGsU || vs.grid != grid) fail(SPK_ERR_STATE, "gs_fused: not the fat vector shape");
    if (b.ar.P || b.sr.n || b.sr.peer) fail(SPK_ERR_STATE, "gs_fused: one rank only");
    if (g.cnt > 40 || b.nv + b.m > kMaxNv - 1) fail(SPK_ERR_ARG, "gs_fused: %d values exceed one reduction", g.cnt);
    b.gmain = (int)grid;
    g.variant = v;
    gs_stamps_aim(b.loc, (int)grid, s);   // (GS_STAMPS=1 builds only)
    gs_dispatch(dot_groups(g.cnt), plane_class(b.m), [&](auto ngc, auto mpc) {
        hipLaunchKernelGGL((gs_kernel<ngc.value, mpc.value>(v)), dim3((unsigned)grid), dim3(kGsT), 0, s, b, g);
    });
    return b.gmain;
}

bool gs_stamps(unsigned long long *out) { return gs_stamps_fetch(out); }

}  // namespace k
}  // namespace spk
