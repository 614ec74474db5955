// The instruction encoder's recurrences for gfx950: nn.LSTM or nn.GRU (MODEL.INSTRUCTION_ENCODER.rnn_type), one or two
// directions (`bidirectional`), length-masked over packed sequences, each with its BPTT.  The reference builds the module
// from the config (ivlnce_baselines/models/encoders/instruction_encoder.py:27-32), runs it over pack_padded_sequence and
// returns pad_packed_sequence(...).permute(0, 2, 1) (:84-94).  Gate order is torch's: i, f, g, o (LSTM) and r, z, n (GRU).
//
//   LSTM  i, f, o = s(gx + W_h. h + b_h.)   g = tanh(gx_g + W_hg h + b_hg)   c' = f c + i g   h' = o tanh(c')
//   GRU   r = s(gi_r + W_hr h + b_hr)   z = s(gi_z + W_hz h + b_hz)   n = tanh(gi_n + r * (W_hn h + b_hn))
//         h' = (1 - z) * n + z * h
//
// gx / gi = W_ih x + b_ih of every position comes from the GEMM (update pass) or from the folded token table (rollout,
// k_embed_gates in nn_ops.hip with G = 4H or 3H).  All fp32.  The two cells share their work split, written once below as
// templates on the gate count NG (no runtime switch on the cell); the element parts - activations, saves, gradient
// formulas - are each kernel's own.  The kernels are plain launches: nothing persistent, no spinning.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/ivln_hip.h"

namespace {

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? IVLN_OK : IVLN_E_HIP)

// DPP quad permutation of a float (ctrl = p0 | p1<<2 | p2<<4 | p3<<6: lane i of each quad reads lane p_i)
template <int CTRL>
__device__ __forceinline__ float quad_perm(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}

// Barrier that orders LDS traffic only.  __syncthreads() also releases GLOBAL stores, i.e. the compiler
// puts s_waitcnt vmcnt(0) in front of it: in a per-timestep loop that also writes its outputs to HBM
// every step then waits for the store acknowledgement.  Nothing in those loops reads global data written
// by the block, so the recurrent kernels order only their LDS traffic.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

typedef float v2f __attribute__((ext_vector_type(2)));

// min(lengths[b], L), and never negative: a negative length would make the tail loops store in front of the row
__device__ __forceinline__ int clamp_len(int len, int L) {
    if (len > L) len = L;
    if (len < 0) len = 0;
    return len;
}

// ------------------------------------------------------------------------------------------
// Forward, both cells.  4H = 512 threads per (sequence, direction).  Quad j (threads 4j..4j+3) owns hidden unit j: lane q
// multiplies the unit's NG gate rows with ITS quarter of h (an NG x H/4 block of W_hh in registers, statically indexed),
// the quad adds the partial sums by DPP so that every lane holds all NG products W_h* h.  Per timestep: H/16 ds_read_b128
// per thread (every thread reading all of h saturated the LDS port), no LDS round trip for gates or cell state and ONE
// LDS-only barrier (h for the next step, double-buffered in hs[2][4 * (H/4 + 4)]: +4 words per quarter, so the 4 quarters
// hit different banks).
// ------------------------------------------------------------------------------------------
template <int NG, int H>
__device__ __forceinline__ void load_quad_weights(v2f (&w)[NG][H / 8], const float* __restrict__ whh, int j, int q) {
#pragma unroll
    for (int r = 0; r < NG; ++r)
#pragma unroll
        for (int k = 0; k < H / 8; ++k) {
            const float* wp = whh + (int64_t)(r * H + j) * H + q * (H / 4) + 2 * k;
            w[r][k] = v2f{wp[0], wp[1]};
        }
}

// ps[r] = (gate row r of unit j) . h for all lanes of the quad; hq = this lane's quarter of h in LDS
template <int NG, int H>
__device__ __forceinline__ void quad_matvec(float (&ps)[NG], const v2f (&w)[NG][H / 8], const float* hq) {
    v2f p[NG];
#pragma unroll
    for (int r = 0; r < NG; ++r) p[r] = v2f{0.f, 0.f};
#pragma unroll
    for (int k = 0; k < H / 4; k += 4) {
        const float4 hv = *reinterpret_cast<const float4*>(&hq[k]);
#pragma unroll
        for (int r = 0; r < NG; ++r) {
            p[r] = __builtin_elementwise_fma(w[r][k / 2], v2f{hv.x, hv.y}, p[r]);
            p[r] = __builtin_elementwise_fma(w[r][k / 2 + 1], v2f{hv.z, hv.w}, p[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < NG; ++r) {
        float v = p[r].x + p[r].y;
        v += quad_perm<0xB1>(v);  // lanes 1,0,3,2
        v += quad_perm<0x4E>(v);  // lanes 2,3,0,1
        ps[r] = v;
    }
}

// step(s, gx_at(s)) for the processing steps s = 0 .. len-1.  gx_at(s), this lane's gate input of step s (one float per
// timestep), is prefetched FOUR steps ahead in a rotating register queue: a timestep is ~0.4 us of work but a fresh HBM row
// costs ~2 us, so a one-step prefetch left every step waiting on memory.
template <class GxAt, class Step>
__device__ __forceinline__ void run_prefetched(int len, GxAt gx_at, Step step) {
    float g0 = gx_at(0), g1 = gx_at(1), g2 = gx_at(2), g3 = gx_at(3);
    for (int s = 0; s < len; s += 4) {
        step(s, g0);
        g0 = gx_at(s + 4);
        if (s + 1 >= len) break;
        step(s + 1, g1);
        g1 = gx_at(s + 5);
        if (s + 2 >= len) break;
        step(s + 2, g2);
        g2 = gx_at(s + 6);
        if (s + 3 >= len) break;
        step(s + 3, g3);
        g3 = gx_at(s + 7);
    }
}

// out is exactly zero for t >= len (orow = the (sequence, direction, unit) row of L floats; lane 0 of the quad writes it)
__device__ __forceinline__ void zero_tail(float* __restrict__ orow, int len, int L) {
    for (int t = len; t < L; ++t) orow[t] = 0.f;
}

// ------------------------------------------------------------------------------------------
// LSTM forward.  ND = direction count (instruction_encoder.py:27-32, `bidirectional`): the grid is ND * B items, item =
// dir * B + b; with ND == 1 every item is a forward one and the *_r pointers are never read.  gx_* (B*L, 4H).  Lane q of
// the quad activates gate q, the quad exchanges the four activations by DPP and every lane updates c / h redundantly (c
// lives in a register).  out (B, ND*H, L) channel-major, exactly zero for t >= min(lengths[b], L).  Optional saves for the
// BPTT: gates (B, ND, L, 4H) post-activation, cs (B, ND, L, H).
// ------------------------------------------------------------------------------------------
template <int H, int ND>
__global__ __launch_bounds__(4 * H) void k_lstm_bidir(const float* __restrict__ gx_f,
                                                      const float* __restrict__ gx_r,
                                                      const float* __restrict__ whh_f,
                                                      const float* __restrict__ whh_r,
                                                      const float* __restrict__ bhh_f,
                                                      const float* __restrict__ bhh_r,
                                                      const int* __restrict__ lengths, int L,
                                                      float* __restrict__ out, float* __restrict__ save_gates,
                                                      float* __restrict__ save_c, int B, unsigned* __restrict__ ticket,
                                                      const int* __restrict__ dirty) {
    constexpr int G = 4 * H;
    // Which (sequence, direction) this block runs: its index, or - with `ticket` - the order in which the blocks START.
    // The launcher then over-subscribes the grid (2B * spare blocks for 2B items): beside a kernel that fills some XCDs
    // (the persistent depth encoder; this kernel's 340 registers per SIMD lane do not fit next to it) the blocks the
    // dispatcher handed to the free XCDs start first and take all the work, the others start when the neighbour ends and
    // leave at once.  The block that draws the last ticket re-arms the counter for the next launch.
    __shared__ int s_item;
    int item = blockIdx.x;
    if (ticket) {
        if (threadIdx.x == 0) {
            const unsigned t = atomicAdd(ticket, 1u);
            if (t == gridDim.x - 1) atomicExch(ticket, 0u);
            s_item = (int)t;
        }
        __syncthreads();
        item = s_item;
        if (item >= ND * B) return;
    }
    if (dirty && !dirty[item % B]) return;  // (per-episode cache, k_embed_gates: this row's output of last step stands)
    constexpr int HQ = H / 4, HQP = HQ + 4;
    __shared__ __attribute__((aligned(16))) float hs[2][4 * HQP];
    const int b = item % B, dir = item / B, tid = threadIdx.x;
    const int q = tid & 3, j = tid >> 2;
    const int g = q * H + j;  // this lane's gate row (PyTorch order i,f,g,o)
    const float* gx = (dir == 0 ? gx_f : gx_r) + (int64_t)b * L * G;
    const float bias = (dir == 0 ? bhh_f : bhh_r)[g];
    v2f w[4][HQ / 2];
    load_quad_weights<4, H>(w, dir == 0 ? whh_f : whh_r, j, q);
    const int hslot = (j / HQ) * HQP + j % HQ;
    if (q == 0) hs[0][hslot] = 0.f;
    float c = 0.f;
    lds_barrier();
    const int len = clamp_len(lengths[b], L);
    auto gx_at = [&](int s) -> float {
        return s < len ? gx[(int64_t)(dir == 0 ? s : len - 1 - s) * G + g] : 0.f;
    };
    run_prefetched(len, gx_at, [&](int s, float gxv) {
        const int t = dir == 0 ? s : len - 1 - s;
        float ps[4];
        quad_matvec<4, H>(ps, w, &hs[s & 1][q * HQP]);
        const float acc = gxv + bias + (q == 0 ? ps[0] : (q == 1 ? ps[1] : (q == 2 ? ps[2] : ps[3])));
        // sigmoid / tanh through one fast exp each (|err| ~1e-7): tanh(x) = 2*sigmoid(2x) - 1
        // (v_rcp_f32 is 1 ulp; an IEEE division is a ~10-instruction sequence on the per-step critical path)
        const float e = __expf(q == 2 ? -2.f * acc : -acc);
        const float rc = __builtin_amdgcn_rcpf(1.f + e);
        const float a = q == 2 ? 2.f * rc - 1.f : rc;
        if (save_gates) save_gates[(((int64_t)b * ND + dir) * L + t) * G + g] = a;
        const float ai = quad_perm<0x00>(a), af = quad_perm<0x55>(a), ag = quad_perm<0xAA>(a), ao = quad_perm<0xFF>(a);
        c = af * c + ai * ag;
        const float h = ao * (2.f * __builtin_amdgcn_rcpf(1.f + __expf(-2.f * c)) - 1.f);
        if (q == 0) {
            hs[(s + 1) & 1][hslot] = h;
            out[((int64_t)b * ND * H + dir * H + j) * L + t] = h;
            if (save_c) save_c[(((int64_t)b * ND + dir) * L + t) * H + j] = c;
        }
        lds_barrier();
    });
    if (q == 0) zero_tail(out + ((int64_t)b * ND * H + dir * H + j) * L, len, L);
}

// ------------------------------------------------------------------------------------------
// GRU forward.  grid nd * B, item = dir * B + b.  gx_* (B*L, 3H).  The quad holds the unit's THREE gate rows (3 x H/4 = 96
// weights per lane).  Lanes 0 and 1 activate r and z (one fast exp each, in the same instruction), the quad exchanges them
// by DPP, then every lane computes n and the new h redundantly (h lives in a register; LDS holds it only for the matvec).
// Lane q < 3 fetches the gate input of row q; lane 3 mirrors lane 2's addresses so that no lane branches around a load.
// out (B, nd*H, L), exactly zero for t >= min(lengths[b], L).  save (optional) (B, nd, L, 4, H): r, z, n, W_hn h + b_hn.
// ------------------------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(4 * H) void k_gru_dirs(const float* __restrict__ gx_f, const float* __restrict__ gx_r,
                                                    const float* __restrict__ whh_f, const float* __restrict__ whh_r,
                                                    const float* __restrict__ bhh_f, const float* __restrict__ bhh_r,
                                                    const int* __restrict__ lengths, int L, int nd,
                                                    float* __restrict__ out, float* __restrict__ save, int B,
                                                    const int* __restrict__ dirty) {
    constexpr int G = 3 * H;
    const int item = blockIdx.x;
    const int b = item % B, dir = item / B, tid = threadIdx.x;
    if (dirty && !dirty[b]) return;  // (per-episode cache, k_embed_gates: this row's output of last step stands)
    constexpr int HQ = H / 4, HQP = HQ + 4;
    __shared__ __attribute__((aligned(16))) float hs[2][4 * HQP];
    const int q = tid & 3, j = tid >> 2;
    const int g = (q < 3 ? q : 2) * H + j;  // the gate row whose input and bias this lane fetches (order r, z, n)
    const float* gx = (dir == 0 ? gx_f : gx_r) + (int64_t)b * L * G;
    const float bias = (dir == 0 ? bhh_f : bhh_r)[g];
    const float bhn = quad_perm<0xAA>(bias);
    v2f w[3][HQ / 2];
    load_quad_weights<3, H>(w, dir == 0 ? whh_f : whh_r, j, q);
    const int hslot = (j / HQ) * HQP + j % HQ;
    if (q == 0) hs[0][hslot] = 0.f;
    float h = 0.f;
    lds_barrier();
    const int len = clamp_len(lengths[b], L);
    float* orow = out + ((int64_t)b * nd * H + dir * H + j) * L;
    float* srow = save ? save + (((int64_t)b * nd + dir) * L * 4 + q) * H + j : nullptr;
    auto gx_at = [&](int s) -> float {
        return s < len ? gx[(int64_t)(dir == 0 ? s : len - 1 - s) * G + g] : 0.f;
    };
    run_prefetched(len, gx_at, [&](int s, float gxv) {
        const int t = dir == 0 ? s : len - 1 - s;
        float ps[3];
        quad_matvec<3, H>(ps, w, &hs[s & 1][q * HQP]);
        const float gin = quad_perm<0xAA>(gxv);
        const float hn = ps[2] + bhn;
        // lanes 0 / 1: r / z (lanes 2, 3 compute a value nobody reads);  sigmoid / tanh through one fast exp each
        const float acc = gxv + bias + (q == 0 ? ps[0] : ps[1]);
        const float a = __builtin_amdgcn_rcpf(1.f + __expf(-acc));
        const float rg = quad_perm<0x00>(a), zg = quad_perm<0x55>(a);
        const float ng = 2.f * __builtin_amdgcn_rcpf(1.f + __expf(-2.f * (gin + rg * hn))) - 1.f;
        h = (1.f - zg) * ng + zg * h;
        if (srow) srow[(int64_t)t * 4 * H] = q == 0 ? rg : (q == 1 ? zg : (q == 2 ? ng : hn));
        if (q == 0) {
            hs[(s + 1) & 1][hslot] = h;
            orow[t] = h;
        }
        lds_barrier();
    });
    if (q == 0) zero_tail(orow, len, L);
}

// ------------------------------------------------------------------------------------------
// BPTT, both cells.  grid (B, directions); 4H = 512 threads.  Threads 0..H-1 own a hidden unit each for the element part
// (its inputs - the forward's saves, dout - are fetched one timestep ahead).  For dh_prev[k] = sum_g W_hh[g][k] dg[g]
// (NG * H terms) thread (ko = tid / 16, ig = tid % 16) owns the 4 outputs k = 4ko..4ko+3 and the RG = NG * H / 16 gate rows
// g = RG*ig .. RG*ig + RG-1 (4 * RG weights in registers), reads ONLY its RG gate gradients from LDS (RG/4 ds_read_b128;
// every thread reading all of them saturated the LDS port), and the 16 lanes that share an output add their partial sums
// by shuffles.  dg is kept in 16 groups of RG floats with stride RG + 4: the groups spread over the banks.  Two LDS-only
// barriers per timestep.  The two kernels share this split in words only: each keeps its own copy of the weight load, the
// zeroing of the padded positions and the matvec with its reduction (why: DESIGN.md, the instruction-encoder paragraph).
// ------------------------------------------------------------------------------------------

// ------------------------------------------------------------------------------------------
// LSTM BPTT (forward: k_lstm_bidir<H, ND>).  grid (B, ND); dout / out (B, ND*H, L), saves (B, ND, L, .).  Writes dgx
// (B*L, 4H) per direction (pre-activation gate grads) and hprev (B*L, H) per direction (h_{t-1} in processing order) for
// the dW_hh / dW_ih GEMMs; both exactly zero for t >= len, dout there is never read.
// ------------------------------------------------------------------------------------------
template <int H, int ND>
__global__ __launch_bounds__(4 * H) void k_lstm_bidir_bwd(const float* __restrict__ dout,
                                                          const float* __restrict__ out,
                                                          const float* __restrict__ gates,
                                                          const float* __restrict__ cs,
                                                          const float* __restrict__ whh_f,
                                                          const float* __restrict__ whh_r,
                                                          const int* __restrict__ lengths, int L,
                                                          float* __restrict__ dgx_f, float* __restrict__ dgx_r,
                                                          float* __restrict__ hprev_f,
                                                          float* __restrict__ hprev_r) {
    constexpr int G = 4 * H;
    constexpr int RG = 32, GS = RG + 4;
    static_assert(H == 128 && G == 16 * RG, "mapping below assumes 512 threads and 512 gate rows");
    __shared__ __attribute__((aligned(16))) float dg[16 * GS];
    __shared__ float dhc[H];
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const int ig = tid & 15, ko = tid >> 4;
    float* dgx = (dir == 0 ? dgx_f : dgx_r) + (int64_t)b * L * G;
    float* hprev = (dir == 0 ? hprev_f : hprev_r) + (int64_t)b * L * H;
    float w[4][RG];
    const float* whh = dir == 0 ? whh_f : whh_r;
#pragma unroll
    for (int g = 0; g < RG; ++g) {
        const float4 v = *reinterpret_cast<const float4*>(whh + (int64_t)(ig * RG + g) * H + ko * 4);
        w[0][g] = v.x, w[1][g] = v.y, w[2][g] = v.z, w[3][g] = v.w;
    }
    if (tid < H) dhc[tid] = 0.f;
    const int len = clamp_len(lengths[b], L);
    {
        const int k = tid % H, pq = tid / H;
        for (int t = len + pq; t < L; t += 4) {  // padded positions carry no gradient
#pragma unroll 4
            for (int g = k; g < G; g += H) dgx[(int64_t)t * G + g] = 0.f;
            hprev[(int64_t)t * H + k] = 0.f;
        }
    }
    lds_barrier();
    const float* gt = gates + ((int64_t)b * ND + dir) * L * G;
    const float* ct = cs + ((int64_t)b * ND + dir) * L * H;
    const int j = tid;  // element part: threads 0..H-1 own hidden unit j
    const int64_t orow = ((int64_t)b * ND * H + dir * H + (j < H ? j : 0)) * L;
    float dcc = 0.f;    // dc carried to the previous timestep (register: only thread j touches it)
    // inputs of a timestep: gates i,f,g,o, c, c_prev, h_prev, dout
    float n_i = 0.f, n_f = 0.f, n_g = 0.f, n_o = 0.f, n_c = 0.f, n_cp = 0.f, n_hp = 0.f, n_do = 0.f;
    auto fetch = [&](int s) {
        if (j < H && s >= 0) {
            const int t = dir == 0 ? s : len - 1 - s, tp = dir == 0 ? t - 1 : t + 1;
            n_i = gt[(int64_t)t * G + j], n_f = gt[(int64_t)t * G + H + j];
            n_g = gt[(int64_t)t * G + 2 * H + j], n_o = gt[(int64_t)t * G + 3 * H + j];
            n_c = ct[(int64_t)t * H + j];
            n_cp = s > 0 ? ct[(int64_t)tp * H + j] : 0.f;
            n_hp = s > 0 ? out[orow + tp] : 0.f;
            n_do = dout[orow + t];
        }
    };
    fetch(len - 1);
    for (int s = len - 1; s >= 0; --s) {
        const int t = dir == 0 ? s : len - 1 - s;  // time index of processing step s
        const float ig_ = n_i, fg = n_f, gg = n_g, og = n_o, c = n_c, cp = n_cp, hp = n_hp, dov = n_do;
        fetch(s - 1);  // next timestep's inputs, in flight under this one
        if (j < H) {
            const float e2 = __expf(-2.f * c);
            const float tc = 2.f * __builtin_amdgcn_rcpf(1.f + e2) - 1.f;  // tanh(c)
            const float dh = dov + dhc[j];
            const float d_o = dh * tc;
            const float dc = dh * og * (1.f - tc * tc) + dcc;
            const float di = dc * gg, df = dc * cp, dgg = dc * ig_;
            dcc = dc * fg;
            const float a0 = di * ig_ * (1.f - ig_), a1 = df * fg * (1.f - fg), a2 = dgg * (1.f - gg * gg),
                        a3 = d_o * og * (1.f - og);
            // gate row q*H + j lives in group (q*H + j) / 32, slot (q*H + j) % 32
            dg[((0 * H + j) >> 5) * GS + (j & 31)] = a0;
            dg[((1 * H + j) >> 5) * GS + (j & 31)] = a1;
            dg[((2 * H + j) >> 5) * GS + (j & 31)] = a2;
            dg[((3 * H + j) >> 5) * GS + (j & 31)] = a3;
            dgx[(int64_t)t * G + j] = a0;
            dgx[(int64_t)t * G + H + j] = a1;
            dgx[(int64_t)t * G + 2 * H + j] = a2;
            dgx[(int64_t)t * G + 3 * H + j] = a3;
            hprev[(int64_t)t * H + j] = hp;
        }
        lds_barrier();
        float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
#pragma unroll
        for (int g = 0; g < RG; g += 4) {
            const float4 v = *reinterpret_cast<const float4*>(&dg[ig * GS + g]);
            p0 = fmaf(w[0][g], v.x, p0), p1 = fmaf(w[1][g], v.x, p1), p2 = fmaf(w[2][g], v.x, p2), p3 = fmaf(w[3][g], v.x, p3);
            p0 = fmaf(w[0][g + 1], v.y, p0), p1 = fmaf(w[1][g + 1], v.y, p1), p2 = fmaf(w[2][g + 1], v.y, p2),
            p3 = fmaf(w[3][g + 1], v.y, p3);
            p0 = fmaf(w[0][g + 2], v.z, p0), p1 = fmaf(w[1][g + 2], v.z, p1), p2 = fmaf(w[2][g + 2], v.z, p2),
            p3 = fmaf(w[3][g + 2], v.z, p3);
            p0 = fmaf(w[0][g + 3], v.w, p0), p1 = fmaf(w[1][g + 3], v.w, p1), p2 = fmaf(w[2][g + 3], v.w, p2),
            p3 = fmaf(w[3][g + 3], v.w, p3);
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {  // the 16 lanes of an output group are consecutive
            p0 += __shfl_xor(p0, off, 64);
            p1 += __shfl_xor(p1, off, 64);
            p2 += __shfl_xor(p2, off, 64);
            p3 += __shfl_xor(p3, off, 64);
        }
        if (ig == 0) {  // dhc of this step was consumed before the first barrier: safe to overwrite
            dhc[ko * 4] = p0;
            dhc[ko * 4 + 1] = p1;
            dhc[ko * 4 + 2] = p2;
            dhc[ko * 4 + 3] = p3;
        }
        lds_barrier();
    }
}

// ------------------------------------------------------------------------------------------
// GRU BPTT (forward: k_gru_dirs).  grid (B, nd).  The direct path dh * z stays in the unit's register.
//   dn = dh (1 - z);  dz = dh (h_prev - n);  a_n = dn (1 - n^2);  a_z = dz z (1 - z);  a_r = a_n ghn r (1 - r)
//   dgi = [a_r, a_z, a_n];  dgh = [a_r, a_z, a_n r];  dh_prev = dh z + W_hh^T dgh
// dgi / dgh (B*L, 3H) and hprev (B*L, H) per direction, exactly zero for t >= len; dout there is never read.
// ------------------------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(4 * H) void k_gru_dirs_bwd(const float* __restrict__ dout, const float* __restrict__ out,
                                                        const float* __restrict__ save, const float* __restrict__ whh_f,
                                                        const float* __restrict__ whh_r, const int* __restrict__ lengths,
                                                        int L, int nd, float* __restrict__ dgi_f, float* __restrict__ dgi_r,
                                                        float* __restrict__ dgh_f, float* __restrict__ dgh_r,
                                                        float* __restrict__ hprev_f, float* __restrict__ hprev_r) {
    constexpr int G = 3 * H;
    constexpr int RG = 24, GS = RG + 4;
    static_assert(H == 128 && G == 16 * RG, "mapping below assumes 512 threads and 384 gate rows");
    __shared__ __attribute__((aligned(16))) float dg[16 * GS];
    __shared__ float dhc[H];
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const int ig = tid & 15, ko = tid >> 4;
    float* dgi = (dir == 0 ? dgi_f : dgi_r) + (int64_t)b * L * G;
    float* dgh = (dir == 0 ? dgh_f : dgh_r) + (int64_t)b * L * G;
    float* hprev = (dir == 0 ? hprev_f : hprev_r) + (int64_t)b * L * H;
    float w[4][RG];
    const float* whh = dir == 0 ? whh_f : whh_r;
#pragma unroll
    for (int g = 0; g < RG; ++g) {
        const float4 v = *reinterpret_cast<const float4*>(whh + (int64_t)(ig * RG + g) * H + ko * 4);
        w[0][g] = v.x, w[1][g] = v.y, w[2][g] = v.z, w[3][g] = v.w;
    }
    if (tid < H) dhc[tid] = 0.f;
    const int len = clamp_len(lengths[b], L);
    {
        const int k = tid % H, pq = tid / H;
        for (int t = len + pq; t < L; t += 4) {
#pragma unroll
            for (int g = k; g < G; g += H) dgi[(int64_t)t * G + g] = 0.f, dgh[(int64_t)t * G + g] = 0.f;
            hprev[(int64_t)t * H + k] = 0.f;
        }
    }
    lds_barrier();
    const float* sv = save + ((int64_t)b * nd + dir) * L * 4 * H;
    const int j = tid;  // element part: threads 0..H-1 own hidden unit j
    const int64_t orow = ((int64_t)b * nd * H + dir * H + (j < H ? j : 0)) * L;
    float dhz = 0.f;  // dh * z carried to the previous timestep (register: only thread j touches it)
    float n_r = 0.f, n_z = 0.f, n_n = 0.f, n_gh = 0.f, n_hp = 0.f, n_do = 0.f;
    auto fetch = [&](int s) {
        if (j < H && s >= 0) {
            const int t = dir == 0 ? s : len - 1 - s, tp = dir == 0 ? t - 1 : t + 1;
            const float* p = sv + (int64_t)t * 4 * H + j;
            n_r = p[0], n_z = p[H], n_n = p[2 * H], n_gh = p[3 * H];
            n_hp = s > 0 ? out[orow + tp] : 0.f;
            n_do = dout[orow + t];
        }
    };
    fetch(len - 1);
    for (int s = len - 1; s >= 0; --s) {
        const int t = dir == 0 ? s : len - 1 - s;  // time index of processing step s
        const float rg = n_r, zg = n_z, ng = n_n, gh = n_gh, hp = n_hp, dov = n_do;
        fetch(s - 1);  // next timestep's inputs, in flight under this one
        if (j < H) {
            const float dh = dov + dhc[j] + dhz;
            const float a_n = dh * (1.f - zg) * (1.f - ng * ng);
            const float a_z = dh * (hp - ng) * zg * (1.f - zg);
            const float a_r = a_n * gh * rg * (1.f - rg);
            const float a_hn = a_n * rg;
            dhz = dh * zg;
            // gate row q*H + j lives in group (q*H + j) / RG, slot (q*H + j) % RG
            dg[((0 * H + j) / RG) * GS + (0 * H + j) % RG] = a_r;
            dg[((1 * H + j) / RG) * GS + (1 * H + j) % RG] = a_z;
            dg[((2 * H + j) / RG) * GS + (2 * H + j) % RG] = a_hn;
            dgi[(int64_t)t * G + j] = a_r;
            dgi[(int64_t)t * G + H + j] = a_z;
            dgi[(int64_t)t * G + 2 * H + j] = a_n;
            dgh[(int64_t)t * G + j] = a_r;
            dgh[(int64_t)t * G + H + j] = a_z;
            dgh[(int64_t)t * G + 2 * H + j] = a_hn;
            hprev[(int64_t)t * H + j] = hp;
        }
        lds_barrier();
        float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
#pragma unroll
        for (int g = 0; g < RG; g += 4) {
            const float4 v = *reinterpret_cast<const float4*>(&dg[ig * GS + g]);
            p0 = fmaf(w[0][g], v.x, p0), p1 = fmaf(w[1][g], v.x, p1), p2 = fmaf(w[2][g], v.x, p2), p3 = fmaf(w[3][g], v.x, p3);
            p0 = fmaf(w[0][g + 1], v.y, p0), p1 = fmaf(w[1][g + 1], v.y, p1), p2 = fmaf(w[2][g + 1], v.y, p2),
            p3 = fmaf(w[3][g + 1], v.y, p3);
            p0 = fmaf(w[0][g + 2], v.z, p0), p1 = fmaf(w[1][g + 2], v.z, p1), p2 = fmaf(w[2][g + 2], v.z, p2),
            p3 = fmaf(w[3][g + 2], v.z, p3);
            p0 = fmaf(w[0][g + 3], v.w, p0), p1 = fmaf(w[1][g + 3], v.w, p1), p2 = fmaf(w[2][g + 3], v.w, p2),
            p3 = fmaf(w[3][g + 3], v.w, p3);
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {  // the 16 lanes of an output group are consecutive
            p0 += __shfl_xor(p0, off, 64);
            p1 += __shfl_xor(p1, off, 64);
            p2 += __shfl_xor(p2, off, 64);
            p3 += __shfl_xor(p3, off, 64);
        }
        if (ig == 0) {  // dhc of this step was consumed before the first barrier: safe to overwrite
            dhc[ko * 4] = p0;
            dhc[ko * 4 + 1] = p1;
            dhc[ko * 4 + 2] = p2;
            dhc[ko * 4 + 3] = p3;
        }
        lds_barrier();
    }
}

}  // namespace

extern "C" {

int ivln_lstm_dirs_fwd_f32(const float* gx_f, const float* gx_r, const float* whh_f, const float* whh_r, const float* bhh_f,
                           const float* bhh_r, const int* lengths, int B, int L, int H, int ndir, float* out,
                           float* save_gates, float* save_c, unsigned* ticket, int spare, const int* dirty, void* stream) {
    if (H != 128) return IVLN_E_UNSUPPORTED;
    if (B <= 0 || L <= 0 || spare < 1 || spare > 8 || (spare > 1 && !ticket) || (ndir != 1 && ndir != 2)) return IVLN_E_INVALID;
    if (!gx_f || !whh_f || !bhh_f || !lengths || !out || (ndir == 2 && (!gx_r || !whh_r || !bhh_r))) return IVLN_E_INVALID;
    if (ndir == 2)
        hipLaunchKernelGGL((k_lstm_bidir<128, 2>), dim3(2 * B * (ticket ? spare : 1)), dim3(512), 0, (hipStream_t)stream, gx_f,
                           gx_r, whh_f, whh_r, bhh_f, bhh_r, lengths, L, out, save_gates, save_c, B, ticket, dirty);
    else
        hipLaunchKernelGGL((k_lstm_bidir<128, 1>), dim3(B * (ticket ? spare : 1)), dim3(512), 0, (hipStream_t)stream, gx_f,
                           gx_f, whh_f, whh_f, bhh_f, bhh_f, lengths, L, out, save_gates, save_c, B, ticket, dirty);
    return LAUNCH_OK();
}

int ivln_lstm_dirs_bwd_f32(const float* dout, const float* out, const float* gates, const float* cs, const float* whh_f,
                           const float* whh_r, const int* lengths, int B, int L, int H, int ndir, float* dgx_f, float* dgx_r,
                           float* hprev_f, float* hprev_r, void* stream) {
    if (H != 128) return IVLN_E_UNSUPPORTED;
    if (B <= 0 || L <= 0 || (ndir != 1 && ndir != 2)) return IVLN_E_INVALID;
    if (!dout || !out || !gates || !cs || !whh_f || !lengths || !dgx_f || !hprev_f) return IVLN_E_INVALID;
    if (ndir == 2 && (!whh_r || !dgx_r || !hprev_r)) return IVLN_E_INVALID;
    if (ndir == 2)
        hipLaunchKernelGGL((k_lstm_bidir_bwd<128, 2>), dim3(B, 2), dim3(512), 0, (hipStream_t)stream, dout, out, gates, cs,
                           whh_f, whh_r, lengths, L, dgx_f, dgx_r, hprev_f, hprev_r);
    else
        hipLaunchKernelGGL((k_lstm_bidir_bwd<128, 1>), dim3(B, 1), dim3(512), 0, (hipStream_t)stream, dout, out, gates, cs,
                           whh_f, whh_f, lengths, L, dgx_f, dgx_f, hprev_f, hprev_f);
    return LAUNCH_OK();
}

int ivln_gru_dirs_fwd_f32(const float* gx_f, const float* gx_r, const float* whh_f, const float* whh_r, const float* bhh_f,
                          const float* bhh_r, const int* lengths, int B, int L, int H, int ndir, float* out, float* save,
                          const int* dirty, void* stream) {
    if (H != 128) return IVLN_E_UNSUPPORTED;
    if (B <= 0 || L <= 0 || (ndir != 1 && ndir != 2)) return IVLN_E_INVALID;
    if (!gx_f || !whh_f || !bhh_f || !lengths || !out || (ndir == 2 && (!gx_r || !whh_r || !bhh_r))) return IVLN_E_INVALID;
    if (ndir == 1) gx_r = gx_f, whh_r = whh_f, bhh_r = bhh_f;  // (never read: every item is a forward one)
    hipLaunchKernelGGL((k_gru_dirs<128>), dim3(ndir * B), dim3(512), 0, (hipStream_t)stream, gx_f, gx_r, whh_f, whh_r, bhh_f,
                       bhh_r, lengths, L, ndir, out, save, B, dirty);
    return LAUNCH_OK();
}

int ivln_gru_dirs_bwd_f32(const float* dout, const float* out, const float* save, const float* whh_f, const float* whh_r,
                          const int* lengths, int B, int L, int H, int ndir, float* dgi_f, float* dgi_r, float* dgh_f,
                          float* dgh_r, float* hprev_f, float* hprev_r, void* stream) {
    if (H != 128) return IVLN_E_UNSUPPORTED;
    if (B <= 0 || L <= 0 || (ndir != 1 && ndir != 2)) return IVLN_E_INVALID;
    if (!dout || !out || !save || !whh_f || !lengths || !dgi_f || !dgh_f || !hprev_f) return IVLN_E_INVALID;
    if (ndir == 2 && (!whh_r || !dgi_r || !dgh_r || !hprev_r)) return IVLN_E_INVALID;
    if (ndir == 1) whh_r = whh_f, dgi_r = dgi_f, dgh_r = dgh_f, hprev_r = hprev_f;  // (never used: grid (B, 1))
    hipLaunchKernelGGL((k_gru_dirs_bwd<128>), dim3(B, ndir), dim3(512), 0, (hipStream_t)stream, dout, out, save, whh_f, whh_r,
                       lengths, L, ndir, dgi_f, dgi_r, dgh_f, dgh_r, hprev_f, hprev_r);
    return LAUNCH_OK();
}

}  // extern "C"
