// opnet_xcd_split_kernels.hip - the head-once persistent OPNet forward (opnet_xcd_kernels.hip) with every fp32 product computed
// as three f16 MFMAs on the matrix pipe (v_mfma_f32_16x16x32_f16) instead of v_mfma_f32_16x16x4_f32 on the fp32 vector lanes.
//
// Why: fp32 MFMA runs at the VALU rate - a phase carries 174 of them per product wave, 5 568 cycles of a
// measured 7 400, and every VALU instruction of the finish wave beside it is taken from that stream.  The f16 instruction does a
// K = 32 block in ~16 cycles on the matrix pipe proper: 69 MFMAs per phase.
//
// The split.  Every operand a (a weight, x, h1, h2, frames_boxes) travels as two f16 planes
//     hi = RN_f16(a)          lo = RN_f16((a - float(hi)) * 2^11)          a ~ hi + lo * 2^-11   (22+ significant bits)
// (2^11 keeps lo in f16's normal range: without it the low halves of weights near 0.04 are subnormal) and a product is
//     a . b ~ hi_a . hi_b  +  2^-11 (hi_a . lo_b + lo_a . hi_b)            fp32 accumulation; lo . lo (2^-22) is dropped
// f16 overflows at 65 504: the two kernels that split the caller's values (weights, boxes) raise abort code 3 on |value| >= 2^15
// or a non-finite value, the forward then leaves at once, y is poisoned and the caller's monitor re-runs the batch on the launch
// chain.  h is bounded by 1 and frames_boxes by max |box|.
//
// What does NOT change against opnet_xcd_forward<true>: the two roles per SIMD, the one s_barrier per phase, the per-CU flags behind
// the LDS arrival counter, local / write-through stores and the placement check, the bounded spins and the abort word, the debug
// bits and the trace stamps, ring and full-history addressing, the rotating head CU and y CU, 1-KiB LDS-DMA pieces.  Only the
// bytes the protocol moves and the product loop differ:
//   * activations are split planes: per 32-k block one 1-KiB hi piece and one 1-KiB lo piece, [k/8][16 clips][8 halfs] = the B
//     operand lane layout of the instruction (lane l: clip l & 15, k = 8 (l >> 4) + j; tools/probes/mfma_f16_layout_probe.hip).
//     x (3 blocks), h1 (8) and h2 (16) keep their byte counts; frames_boxes is one block (2 KiB, k >= 6 zero - written by the pack
//     kernel once per launch, publishers never write there); the gather is 56 pieces.  No fp32 copy of h exists any more;
//     the fp32 image of x stays for the head wave's einsum, which is exact as before.  c stays fp32 in LDS.
//   * weights are split A fragments (lane l: row l & 15, k = 8 (l >> 4) + j), derived from the packed fp32 image into the
//     workspace before EVERY launch (opnet_xcd_split_weights: 5.7 MB; training updates weights in place, nothing is cached).  A
//     pair of fp32 hexadecet fragments becomes one block's hi and lo fragment: the register count per weight is unchanged.
//
// Summation order (differs from the fp32 kernel's; both are held to the fp64 oracle):
//   every product = fmaf(corr, 2^-11, main), main = sum over blocks (ascending) of hi.hi, corr = sum over blocks (ascending) of
//   (hi_a.lo_b then lo_a.hi_b), each MFMA a K = 32 dot product in the matrix pipe's internal order.
//   LSTM2 gate: blocks 0..15 of h2, then the frames_boxes block.  LSTM1 gate = (blocks 0..5: x, h1[0..95]) + (blocks 6..10), each
//   half its own fmaf(corr, 2^-11, main).  logits: blocks 0..7 on one wave.  y = ((w0 + w1) + w2) + w3 over the product waves, wave
//   w blocks w, w+4, w+8, w+12.  frames_boxes: unchanged (fp32 einsum).
//
// Who issues the gather (four or more groups on the XCD; OPNET_XCD_PGATHER=0 restores the finish waves' early gather).  The 56 KiB of
// LDS-DMA per phase block at issue on the full queue, ~1 720 cycles a phase, and used to sit in front of the finish wave's
// head / cells / drain chain while the product wave of the same SIMD idled for 2 900 cycles.  Now finish wave 0, at the end of its
// phase's work, looks ONCE at the 32 flags of the gather two barriers ahead and posts the verdict in sPG[parity]; both roles read
// the word right after the barrier.  Ready: the product wave issues its first XS_PG_NP pieces behind its MFMA blocks and waits
// vmcnt(0) before its barrier, the finish wave issues the rest and goes on.  Not ready: the finish waves poll and gather at the end
// of the phase exactly as before (bounded spin, abort word) - product waves never look at global memory.  Never ready on the CU
// whose finish wave 0 reads h1 for the selection head out of that buffer, nor where the product waves compute the output head
// (2 phases in 32 per CU).  No arithmetic moves: y and logits are bit-identical (tests/test_opnet_xcd_pgather_gpu.py).
#define XS_SCALE 2048.f
#define XS_ISCALE (1.f / 2048.f)
#define XS_RANGE 32768.f
#define XS_ABORT_RANGE 3u
#define XS_CHUNKS 56
#define XS_F8 (XS_CHUNKS * 64)       // gather buffer in 16-byte units
#define XS_H1 (6 * 64)
#define XS_H2 (22 * 64)

typedef _Float16 xs_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 xs_h4 __attribute__((ext_vector_type(4)));
typedef unsigned xs_u32x2 __attribute__((ext_vector_type(2)));

struct XcdSplitArgs {
    XcdArgs a;                 // first: the finish waves fetch its pointers from the kernarg segment by offset (XCD_KARG).  a.fb_off is the
                               // offset of the 2-KiB frames_boxes slots, a.xp / a.xp_off the fp32 image of x
    const char *wsp;           // split image of the weights: the packed image's offsets (in bytes), a hexadecet pair -> [hi | lo] fragments;
                               // the (unused) W_ih2 region holds one range word per block of opnet_xcd_split_weights
    unsigned xs_off;           // split planes of x in the workspace: [NGT][T+2][3 blocks][hi | lo][64 lanes][8 halfs]
    unsigned wsp_blocks;       // grid of opnet_xcd_split_weights
    int pgather;               // OPNET_XCD_PGATHER (default 1): with four or more groups on an XCD the PRODUCT waves issue the phase
                               // gather a finish wave has found ready; 0: the finish waves issue every gather themselves
};

__device__ __forceinline__ void xs_split(float v, _Float16 *hi, _Float16 *lo)
{
    const _Float16 h = (_Float16)v;
    *hi = h;
    *lo = (_Float16)((v - (float)h) * XS_SCALE);
}
__device__ __forceinline__ bool xs_in_range(float v) { return fabsf(v) < XS_RANGE; }   // false for NaN and infinities too

// packed fp32 image -> split A fragments, and the launch's status words.  One thread per (hexadecet pair, lane): lane (row i, u) of
// block b holds k = 32 b + 8 u + j = element j & 3 of lane (i, 2 (u & 1) + (j >> 2)) of hexadecet 2 b + (u >> 1).
// Every block leaves "a value out of f16 range" in its own word (no word is written by two blocks: no zeroing pass needed);
// opnet_xcd_pack_input_split folds them into status[0].
__global__ void __launch_bounds__(256) opnet_xcd_split_weights(const XcdSplitArgs s)
{
    const PackedLayout P = packed_layout(XCD_H1, XCD_H2);
    const long pairs_a = (long)(P.wih2p / 512), pairs = pairs_a + (long)((P.total - P.wselp) / 512);
    const long i = blockIdx.x * 256L + threadIdx.x;
    bool bad = false;
    if (i < pairs * 64) {
        const long pi = i >> 6;
        const int l = (int)(i & 63), r = l & 15, u = l >> 4;
        const size_t base = (pi < pairs_a ? (size_t)pi * 512 : P.wselp + (size_t)(pi - pairs_a) * 512);   // in floats
        const float4 *src = (const float4 *)(s.a.packed + base + (u >> 1) * 256) + r + 32 * (u & 1);
        const float4 v0 = src[0], v1 = src[16];
        const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        xs_h8 hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            _Float16 h, q;
            xs_split(v[j], &h, &q);
            hi[j] = h; lo[j] = q;
            bad |= !xs_in_range(v[j]);
        }
        xs_h8 *dst = (xs_h8 *)(s.wsp + base * 4) + l;
        dst[0] = hi;
        dst[64] = lo;
    }
    // W_ih2 (split inside the forward, by the product wave that holds it): range only
    if (i < (long)(P.wselp - P.wih2p)) bad |= !xs_in_range(s.a.packed[P.wih2p + i]);
    const int any = __syncthreads_or(bad ? 1 : 0);
    if (threadIdx.x == 0) ((unsigned *)(s.wsp + P.wih2p * 4))[blockIdx.x] = any ? 1u : 0u;
    if (blockIdx.x == 0) {
        if (threadIdx.x < 8) s.a.status[threadIdx.x] = 0u;
        s.a.status[8 + threadIdx.x] = 0xffffffffu;             // XCD_COUNT * XCD_CUS = 256 placement words
    }
}

// boxes -> the fp32 image xp (as opnet_xcd_pack_input) AND the split planes of x; zero slot 0 of the histories, every
// frames_boxes slot (their padding lanes must hold finite zeros) and the flags; fold the range words into status[0] (zeroed by
// opnet_xcd_split_weights, which runs before this kernel).   grid (T + 2, NGT), 384 threads (24 k-quads x 16 clips)
__global__ void __launch_bounds__(384) opnet_xcd_pack_input_split(const XcdSources src, const XcdSplitArgs s)
{
    const XcdArgs &a = s.a;
    const int slot = blockIdx.x, gg = blockIdx.y;
    const int T = a.T, tid = threadIdx.x;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    bool bad = false;
    {
        const int kq = tid % OPNET_KXQ, clip = tid / OPNET_KXQ;
        const int b = gg * 16 + clip, t = slot - 1;
        float4 v = z;
        if (b < a.B && t >= 0 && t < T) {
            int r = 0;
            while (r + 1 < src.n && b >= src.start[r + 1]) ++r;
            const float2 *s2 = (const float2 *)(src.p[r] + ((long)(b - src.start[r]) * T + t) * OPNET_KX + kq * 4);
            const int k = kq * 4;
            if (k + 1 < OPNET_KX) { float2 p = s2[0]; v.x = p.x; v.y = p.y; }
            if (k + 3 < OPNET_KX) { float2 q = s2[1]; v.z = q.x; v.w = q.y; }
        }
        const long sl = (long)gg * (T + 2) + slot;
        ((float4 *)a.xp)[(sl * OPNET_KXQ + kq) * 16 + clip] = v;
        xs_h4 hi, lo;
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            _Float16 h, q;
            xs_split(vv[j], &h, &q);
            hi[j] = h; lo[j] = q;
            bad |= !xs_in_range(vv[j]);
        }
        // k = 4 kq + j: block kq >> 3, lane group (kq >> 1) & 3, halfs 4 (kq & 1) + j
        char *d = a.ws + s.xs_off + sl * (OPNET_KXQ * 256) + (kq >> 3) * 2048 + ((((kq >> 1) & 3) * 16 + clip) * 16) + (kq & 1) * 8;
        *(xs_h4 *)d = hi;
        *(xs_h4 *)(d + 1024) = lo;
    }
    const long NS = a.ring ? XCD_RING : T + 1;                 // slots per group
    for (long fs = slot; fs < NS; fs += T + 2)
        if (tid < 128) ((float4 *)(a.ws + a.fb_off))[((long)gg * NS + fs) * 128 + tid] = z;
    if (slot == 0) {
        float4 *h1 = a.h1h + (long)gg * NS * (XCD_H1 * 4);
        float4 *h2 = a.h2h + (long)gg * NS * (XCD_H2 * 4);
        for (int i = tid; i < XCD_H1 * 4; i += 384) h1[i] = z;
        for (int i = tid; i < XCD_H2 * 4; i += 384) h2[i] = z;
        if (tid < XCD_CUS) a.flags[gg * XCD_CUS + tid] = 0u;
        if (gg == 0) {
            const PackedLayout P = packed_layout(XCD_H1, XCD_H2);
            const unsigned *wb = (const unsigned *)(s.wsp + P.wih2p * 4);
            for (unsigned i = tid; i < s.wsp_blocks; i += 384) bad |= wb[i] != 0u;
        }
    }
    if (__syncthreads_or(bad ? 1 : 0) && tid == 0) atomicMax(a.status, XS_ABORT_RANGE);
}

// 8-byte exchange store (as xcd_store16)
__device__ __forceinline__ void xs_store8(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, xs_u32x2 v, bool local)
{
    if (local) __builtin_amdgcn_raw_buffer_store_b64(v, r, voff, soff, 0);
    else __builtin_amdgcn_raw_buffer_store_b64(v, r, voff, soff, 16);
}

#define XS_MFMA(a_, b_, c_) __builtin_amdgcn_mfma_f32_16x16x32_f16(a_, b_, c_, 0, 0, 0)

// One wave's share (pieces w, w + 4, ...) of the gather of phase (group gi, step s) into LDS buffer `buf`: x = pieces 0..5,
// h1 = 6..21, h2 = 22..53, frames_boxes = 54, 55.  The wave-uniform byte offsets, and piece 4 j + w by itself (j a constant after
// unrolling) - the finish waves issue the 14 pieces in a row, the product waves one behind each block of their MFMAs.
struct XsGather {
    unsigned dst, ox0, oh1, oh2, ofb;
};
__device__ __forceinline__ XsGather xs_gather_of(const XcdSplitArgs &sa, unsigned lds0, unsigned g0, unsigned NS, unsigned smask, int gi, int s,
                                                 int buf, int w)
{
    const XcdArgs &a = sa.a;
    const int T = a.T;
    const unsigned gg = g0 + gi;
    XsGather o;
    o.dst = lds0 + (unsigned)buf * (XS_F8 * 16) + w * 1024;
    o.ox0 = sa.xs_off + ((gg * (T + 2) + (s < T ? s + 1 : T + 1)) * OPNET_KXQ) * 256 + w * 1024;
    o.oh1 = a.h1_off + ((gg * NS + ((unsigned)(s <= T ? s : T) & smask)) * (XCD_H1 / 4)) * 256 + w * 1024;
    o.oh2 = a.h2_off + ((gg * NS + ((unsigned)(s > 2 ? s - 2 : 0) & smask)) * (XCD_H2 / 4)) * 256 + w * 1024;
    o.ofb = a.fb_off + (gg * NS + ((unsigned)(s > 1 ? s - 1 : 0) & smask)) * 2048 + w * 1024;
    return o;
}
__device__ __forceinline__ void xs_gather_piece(__amdgpu_buffer_rsrc_t rws, unsigned lane16, const XsGather &o, int j, int w)
{
    // (each base holds + w KiB; the piece's place inside its region is a constant here, so that no "base - 22 KiB" lives in an SGPR)
    const int q = 4 * j;
    if (q + 3 < 6) xcd_glds16(rws, lane16, o.ox0 + q * 1024, o.dst + q * 1024);
    else if (q >= 6 && q + 3 < 22) xcd_glds16(rws, lane16, o.oh1 + (q - 6) * 1024, o.dst + q * 1024);
    else if (q >= 22 && q + 3 < 54) xcd_glds16(rws, lane16, o.oh2 + (q - 22) * 1024, o.dst + q * 1024);
    else if (q + w < 6) xcd_glds16(rws, lane16, o.ox0 + q * 1024, o.dst + q * 1024);
    else if (q + w < 22) xcd_glds16(rws, lane16, o.oh1 + (q - 6) * 1024, o.dst + q * 1024);
    else if (q + w < 54) xcd_glds16(rws, lane16, o.oh2 + (q - 22) * 1024, o.dst + q * 1024);
    else xcd_glds16(rws, lane16, o.ofb + (q - 54) * 1024, o.dst + q * 1024);
}
// The steady kernel's gather (opnet_xcd_forward_split<true, .>).  A piece is 3 instructions instead of xcd_glds16's 7: m0 = dst + 4 j KiB,
// soffset = base + 4 j KiB, the load.  m0 is neither saved nor restored - the compiler has no use for it in this kernel (no LDS-DMA
// builtin, no s_movrel, no GWS: check the assembly after a change to the kernel) - and the second s_add is the wait state between
// the write of m0 and the load that reads it.  No piece carries a region compare: base[r] is region r's offset MINUS the region's
// first piece, so that piece q = 4 j + w reads base[r] + 4 j KiB whatever r is, and the three pieces whose region depends on the
// wave (j = 1: x | h1, j = 5: h1 | h2, j = 13: h2 | frames_boxes) take their base from one select per gather (c1, c5, c13).
struct XsGatherS {
    unsigned dst, x, h1, h2, c1, c5, c13;
};
__device__ __forceinline__ XsGatherS xs_gather_steady_of(const XsGather &o, int w)
{
    XsGatherS g;
    const bool hi = w >= 2;
    g.dst = o.dst; g.x = o.ox0; g.h1 = o.oh1 - 6 * 1024; g.h2 = o.oh2 - 22 * 1024;
    g.c1 = hi ? g.h1 : g.x;
    g.c5 = hi ? g.h2 : g.h1;
    g.c13 = hi ? o.ofb - 54 * 1024 : g.h2;
    return g;
}
template <int J>
__device__ __forceinline__ void xs_piece(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned src, unsigned dst)
{
    if (J == 0) {
        asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen sc1 lds"
                     :: "v"(voff), "s"(rsrc), "s"(src), "s"(dst) : "memory");
    } else {
        unsigned t;
        asm volatile("s_add_u32 m0, %4, %5\n\ts_add_u32 %0, %3, %5\n\tbuffer_load_dwordx4 %1, %2, %0 offen sc1 lds"
                     : "=&s"(t) : "v"(voff), "s"(rsrc), "s"(src), "s"(dst), "n"(J * 4096) : "memory", "scc");
    }
}
__device__ __forceinline__ void xs_gather_piece_steady(__amdgpu_buffer_rsrc_t rws, unsigned lane16, const XsGatherS &g, int j)
{
    switch (j) {                               // j is a constant after unrolling: one case survives
    case 0: xs_piece<0>(rws, lane16, g.x, g.dst); break;
    case 1: xs_piece<1>(rws, lane16, g.c1, g.dst); break;
    case 2: xs_piece<2>(rws, lane16, g.h1, g.dst); break;
    case 3: xs_piece<3>(rws, lane16, g.h1, g.dst); break;
    case 4: xs_piece<4>(rws, lane16, g.h1, g.dst); break;
    case 5: xs_piece<5>(rws, lane16, g.c5, g.dst); break;
    case 6: xs_piece<6>(rws, lane16, g.h2, g.dst); break;
    case 7: xs_piece<7>(rws, lane16, g.h2, g.dst); break;
    case 8: xs_piece<8>(rws, lane16, g.h2, g.dst); break;
    case 9: xs_piece<9>(rws, lane16, g.h2, g.dst); break;
    case 10: xs_piece<10>(rws, lane16, g.h2, g.dst); break;
    case 11: xs_piece<11>(rws, lane16, g.h2, g.dst); break;
    case 12: xs_piece<12>(rws, lane16, g.h2, g.dst); break;
    default: xs_piece<13>(rws, lane16, g.c13, g.dst); break;
    }
}
// a 32-bit kernel argument fetched where it is used (as XCD_KARG): what one finish wave in 128 needs per phase, or only a wait that
// does not end at once, holds no SGPR across the finish waves' loop - the loop sits at the SGPR limit, and one spilled SGPR
// reserves a VGPR for its lanes in the whole kernel, which the product waves' weights do not have
template <unsigned OFF>
__device__ __forceinline__ unsigned xs_karg_u32()
{
    unsigned v;
    asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(__builtin_amdgcn_kernarg_segment_ptr()), "n"(OFF) : "memory");
    return v;
}
#define XS_KARG32(field) xs_karg_u32<(unsigned)__builtin_offsetof(XcdArgs, field)>()
// Of a wave's 14 pieces of a gather found ready, the product wave issues the first XS_PG_NP, one behind each of its first MFMA
// blocks, and the finish wave of the same SIMD the rest right after the barrier.  Every issue blocks on the full DMA queue, in
// whichever wave it sits: all 14 on the product wave and ITS chain bounds the phase (products + issue 3 340 cycles of a period of
// 3 924 at 640 clips), 8 and both chains end together (period 3 552; 10: 3 556, 6: 3 692; all 14 up front, before the first MFMA:
// 3 876 and the loop spills).  DESIGN.md section 3a.
#ifndef XS_PG_NP
#define XS_PG_NP 8
#endif
// XS_ELOOK 1 (a measured variant, NOT the default: DESIGN_HISTORY.md section 7): finish wave 0 requests the flags for its NEXT verdict
// right after posting this one, so that the load is in flight across the barrier and the value is read behind the vmcnt(0) of the next
// drain; where it does not show all 32 flags the late look follows as without it.  Flags only grow, so what an earlier look saw is still
// there, and the buffer a gather fills is released by the barrier, not by the look.  It does not pay: of the ~750 cycles the late look
// takes on wave 0's chain only 130-250 are the load's round trip - the rest is the issue of the verdict's ~40 instructions behind the
// product wave's MFMAs, where every instruction of a finish wave costs ~15 cycles, the early load's own among them.  0 compiles to the
// kernel without it, instruction for instruction.
#ifndef XS_ELOOK
#define XS_ELOOK 0
#endif
// The steady kernel's finish wave issues its pieces XS_PG_NP .. 13 of a gather found ready as ONE statement (no pad between two
// statements; m0 and the offset advance by 4 KiB a piece): pieces up to 12 lie in h2, 13 takes the wave's corner base.
#if XS_PG_NP == 8
#define XS_RUN_MIDS XS_RUN_MID XS_RUN_MID XS_RUN_MID XS_RUN_MID
#elif XS_PG_NP == 7
#define XS_RUN_MIDS XS_RUN_MID XS_RUN_MID XS_RUN_MID XS_RUN_MID XS_RUN_MID
#elif XS_PG_NP == 6
#define XS_RUN_MIDS XS_RUN_MID XS_RUN_MID XS_RUN_MID XS_RUN_MID XS_RUN_MID XS_RUN_MID
#endif
#define XS_RUN_LOAD "buffer_load_dwordx4 %1, %2, %0 offen sc1 lds\n\t"
#define XS_RUN_MID "s_add_u32 m0, m0, 0x1000\n\ts_add_u32 %0, %0, 0x1000\n\t" XS_RUN_LOAD
__device__ __forceinline__ void xs_gather_finish_run(__amdgpu_buffer_rsrc_t rws, unsigned lane16, const XsGatherS &g)
{
#ifdef XS_RUN_MIDS
    unsigned t;
    asm volatile("s_add_u32 m0, %5, %6\n\ts_add_u32 %0, %3, %6\n\t" XS_RUN_LOAD XS_RUN_MIDS
                 "s_add_u32 m0, m0, 0x1000\n\ts_add_u32 %0, %4, %7\n\t" XS_RUN_LOAD
                 : "=&s"(t) : "v"(lane16), "s"(rws), "s"(g.h2), "s"(g.c13), "s"(g.dst), "n"(XS_PG_NP * 4096), "n"(13 * 4096) : "memory", "scc");
#else
#pragma unroll
    for (int j = XS_PG_NP; j < XS_CHUNKS / 4; ++j) xs_gather_piece_steady(rws, lane16, g, j);
#endif
}
// wave-uniform condition bit of the finish waves' loop, beside XCD_CF_*: the product waves issue the gathers found ready
#define XS_CF_PG 1024u

// the persistent kernel, head-once form, inference: see opnet_xcd_forward for the roles and the protocol.
//
// Three instantiations <STEADY, TRACE> (the kernel itself is the template: its body as an inlined function of a reference to the
// arguments reads them through a generic pointer, and the general kernel then spills a weight fragment):
//   <false, true>  general: every switch at run time, as ever
//   <true, false>  steady: what a busy server and the benchmark run - four or more groups on EVERY XCD, ring layout, product-wave
//                  gather, no debug bit, no trace buffer - all of that compiled in (the host routes: xcd_steady_form in opnet_abi.hip)
//   <true, true>   steady with the stamp sites live, so that a trace measures the kernel that ships
// STEADY removes instructions, never arithmetic: the finish chain is bound by instruction issue behind the product waves' MFMAs
// (~15 cycles an instruction).  Gone from its loops: the stamp tests, the debug tests, the ng == 1 barrier, the
// pre-pgather early-gather arm, the `ahead` / gn / sn loop, the multiplies of the ring offsets (NS = 4: shifts) and of the head-CU /
// y-CU tests (a counter carried with the phase), and 4 of a DMA piece's 7 instructions.  The late path - poll with the bounded spin,
// abort word, gather - the sH1done wait, the range refusal and the placement check are the same code in all three.
template <bool STEADY, bool TRACE>
__global__ void __launch_bounds__(512, 2) opnet_xcd_forward_split(const XcdSplitArgs sa)
{
    const XcdArgs &a = sa.a;
    __shared__ __attribute__((aligned(1024))) xs_h8 sbuf[2][XS_F8];
    __shared__ __attribute__((aligned(16))) float4 sHAND[2][4][XH_F4];
    __shared__ __attribute__((aligned(16))) _Float16 sTR[4][2][2][64];   // (wave, cell, plane): (clip, unit) -> 4 halfs per clip
    __shared__ float sC2[XCD_NGMAX][4][64];
    __shared__ float sC1[XCD_NGMAX][2][64];
    __shared__ int sAbort, sLocal, sH1done;
    __shared__ int sPG[2];                    // [fp & 1]: the gather of phase fp + 2 is ready and the product waves issue it after barrier fp
    __shared__ unsigned sArrive[2];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w = wv & 3;
    const int x = blockIdx.x & (XCD_COUNT - 1), c = blockIdx.x >> 3;
    const int T = a.T;
    int g0, ng;
    xcd_groups(a.NGT, x, &g0, &ng);
    if (ng > XCD_NGMAX) ng = XCD_NGMAX;

    const int n = lane & 15, u = lane >> 4;
    const int t2 = 4 * c + w;                 // LSTM2 tile of this SIMD
    const int t1 = 2 * c + (w >> 1), kh = w & 1;
    // steps 0 .. T+1 = LSTM1 step s | head step s-1 on ONE wave of the XCD | LSTM2 step s-2; ring mode: one more step for y[T-1]
    const bool YH = STEADY || a.ring != 0;
    const int nph = (YH ? T + 3 : T + 2) * ng;
    const PackedLayout P = packed_layout(XCD_H1, XCD_H2);
    if (wv == XCD_FW0) {
        // a value out of f16 range (abort code 3 from the split kernels): every workgroup leaves at once, nobody waits for anybody
        const bool refused = __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
        const int loc = refused ? -1 : (ng > 0 ? xcd_group_is_local(a.status, x) : 0);
        if (ng == 0) {
            if (lane == 0 && !refused)
                __hip_atomic_store(a.status + 8 + blockIdx.x, __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11)) & 0xf,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (lane == 0) {
            XCD_LDS_ST(sLocal, loc > 0 && a.force_safe == 0);
            XCD_LDS_ST(sAbort, loc < 0);
            sArrive[0] = 0u; sArrive[1] = 0u;
            XCD_LDS_ST(sH1done, 0);
            XCD_LDS_ST(sPG[0], 0); XCD_LDS_ST(sPG[1], 0);
            if (loc == 0 && c == 0) atomicAdd(a.status + 3, 1u);
        }
    }
    if (ng == 0) return;
    for (int i = tid; i < XCD_NGMAX * 4 * 64; i += 512) (&sC2[0][0][0])[i] = 0.f;
    for (int i = tid; i < XCD_NGMAX * 2 * 64; i += 512) (&sC1[0][0][0])[i] = 0.f;

    if ((wv >= 4) == (XCD_FW0 == 0)) {
        // =========================================== product waves ===================================================
        // LSTM2: 16 blocks of h2 + the frames_boxes block (W_ih2, K = 6 -> 32: split here, lanes u > 0 zero); LSTM1: blocks
        // 0..5 (lower-K wave) / 6..10 (upper-K wave: its sixth fragment stays zero and is never issued)
        xs_h8 a2h[17], a2l[17], a1h[6], a1l[6];
        {
            const xs_h8 *p2 = (const xs_h8 *)(sa.wsp + P.w2p * 4) + (long)t2 * 32 * 64 + lane;
#pragma unroll
            for (int q = 0; q < 16; ++q) { a2h[q] = p2[(2 * q) * 64]; a2l[q] = p2[(2 * q + 1) * 64]; }
            const float *px = a.packed + P.wih2p + ((long)(4 * t2 + (n >> 2)) * 4 + (n & 3)) * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                _Float16 h, q;
                xs_split(u == 0 ? px[j] : 0.f, &h, &q);
                a2h[16][j] = h; a2l[16][j] = q;
            }
            const xs_h8 *p1 = (const xs_h8 *)(sa.wsp + P.w1p * 4) + ((long)t1 * 22 + 12 * kh) * 64 + lane;
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                if (q < 5 || !kh) { a1h[q] = p1[(2 * q) * 64]; a1l[q] = p1[(2 * q + 1) * 64]; }
                else { a1h[q] = (xs_h8)(_Float16)0; a1l[q] = (xs_h8)(_Float16)0; }
            }
            // The weights count as arrived HERE.  Left to the compiler, the waits for these loads sit in the product loop before each
            // fragment's first MFMA (vmcnt(9) .. vmcnt(0)) - nothing to wait for after phase 0, until this wave has its own DMA in
            // flight there: a vmcnt(0) in the fifth block would then wait out the first pieces of every phase's gather.
#pragma unroll
            for (int q = 0; q < 17; ++q) asm volatile("" :: "v"(a2h[q]), "v"(a2l[q]));
#pragma unroll
            for (int q = 0; q < 6; ++q) asm volatile("" :: "v"(a1h[q]), "v"(a1l[q]));
        }
        const bool mtracer = TRACE && a.trace && blockIdx.x == 0 && tid == (4 - XCD_FW0) * 64;
        // output head: split A fragments of W_out (rows 0..3 of a 16-row tile), fetched on demand (once in 32 phases on a CU)
        const __amdgpu_buffer_rsrc_t rwy = __builtin_amdgcn_make_buffer_rsrc((void *)(sa.wsp + P.woutp * 4), 0, (XCD_H2 / 16) * 1024, 0x00020000);
        const unsigned ylane = lane * 16;
        auto yfrag = [&](int piece) -> xs_h8 {     // 1-KiB piece (wave-uniform): 2 b = hi, 2 b + 1 = lo of block b
            const xcd_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rwy, ylane, (unsigned)piece * 1024u, 0);
            return __builtin_bit_cast(xs_h8, v);
        };
        // the gather of the NEXT phase, issued from here when a finish wave has found it ready (sPG; four or more groups): this
        // wave's first XS_PG_NP pieces go out one behind each of the first blocks' MFMAs (the finish wave issues the rest).  The issue
        // blocks on the full DMA queue - the per-CU L2 -> LDS floor is about the length of the products - and this wave used to idle
        const bool pg = STEADY || (sa.pgather != 0 && ng >= 4);
        const unsigned pNS = STEADY || a.ring ? (unsigned)XCD_RING : (unsigned)(T + 1);
        const unsigned psmask = STEADY || a.ring ? (unsigned)(XCD_RING - 1) : 0xffffffffu;
        const unsigned plds0 = (unsigned)(unsigned long long)(const void *)&sbuf[0][0];
        const __amdgpu_buffer_rsrc_t prws = __builtin_amdgcn_make_buffer_rsrc((void *)a.ws, 0, 0x7fffffff, 0x00020000);
        __syncthreads();                        // phase 0's gather has landed
        if (XCD_LDS_LD(sAbort)) return;
        int pgi = 0, ps = 0;                    // phase p = ps * ng + pgi
        // steady: ps + 11 pgi, carried with the phase - xcd_y_cu(ps, pgi) = (pcu + 16) & 31 without the multiply
        int pcu = 0;
        const int pcu_wrap = 1 - 11 * (ng - 1);
        for (int p = 0; p < nph; ++p) {
            const bool ycu = YH && ps >= 3 && (STEADY ? ((pcu + 16) & (XCD_CUS - 1)) : xcd_y_cu(ps, pgi)) == c;
            const xs_h8 *F = &sbuf[p & 1][0] + lane;
            const xs_h8 *F2 = F + XS_H2;                    // h2 blocks 0..15, then the frames_boxes block
            const xs_h8 *FL = F + (kh ? 12 * 64 : 0);       // [x | h1] blocks 0..5 / 6..10
            if (mtracer) a.trace[(long)p * 8 + 0] = clock64();
            // the verdict posted before barrier p - 1.  (After an abort the finish waves are gone and the word is stale: the
            // phases run out on stale LDS as before, and the bound on p keeps a stale "ready" inside the workspace's slots.)
            const bool issue = pg && !ycu && p >= 1 && p + 1 < nph && __builtin_amdgcn_readfirstlane(XCD_LDS_LD(sPG[(p - 1) & 1])) != 0;
            XsGather go = {};
            XsGatherS gs = {};
            if (issue) {
                const bool wrap = pgi + 1 == ng;
                go = xs_gather_of(sa, plds0, g0, pNS, psmask, wrap ? 0 : pgi + 1, wrap ? ps + 1 : ps, (p + 1) & 1, w);
                if (STEADY) gs = xs_gather_steady_of(go, w);
            }
            f32x4 m2 = {0.f, 0.f, 0.f, 0.f}, c2 = m2, m1 = m2, c1 = m2;
            auto products = [&](auto yk) {
                constexpr bool YK = decltype(yk)::value;    // this CU computes the output head in this phase
                f32x4 my = {0.f, 0.f, 0.f, 0.f}, cy = my;
                xs_h8 ayh, ayl;
                if (YK) { ayh = yfrag(2 * w); ayl = yfrag(2 * w + 1); }
                // B fragments one block (3 or 6 MFMAs) ahead; the order is pinned with sched_barrier after every block - left
                // alone, the scheduler fetches each block right before its MFMAs and every block waits out an LDS round trip.
                // (The upper-K wave's prefetch of "block 5" reads the first h2 pieces: valid LDS, never used.)
                xs_h8 bh[2], bl[2], xh[2], xl[2];
                bh[0] = F2[0]; bl[0] = F2[64]; xh[0] = FL[0]; xl[0] = FL[64];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 17; ++j) {
                    const int cur = j & 1, nxt = cur ^ 1;
                    if (j + 1 < 17) { bh[nxt] = F2[(2 * j + 2) * 64]; bl[nxt] = F2[(2 * j + 3) * 64]; }
                    if (j + 1 < 6) { xh[nxt] = FL[(2 * j + 2) * 64]; xl[nxt] = FL[(2 * j + 3) * 64]; }
                    if (!YK) __builtin_amdgcn_sched_barrier(0);     // (the output head's variant has no registers left for a full second set)
                    m2 = XS_MFMA(a2h[j], bh[cur], m2);
                    c2 = XS_MFMA(a2h[j], bl[cur], c2);
                    if (j < 5 || (j == 5 && !kh)) {
                        m1 = XS_MFMA(a1h[j], xh[cur], m1);
                        c1 = XS_MFMA(a1h[j], xl[cur], c1);
                    }
                    c2 = XS_MFMA(a2l[j], bh[cur], c2);
                    if (j < 5 || (j == 5 && !kh)) c1 = XS_MFMA(a1l[j], xh[cur], c1);
                    if (YK && j < 16 && (j & 3) == w) {
                        my = XS_MFMA(ayh, bh[cur], my);
                        cy = XS_MFMA(ayh, bl[cur], cy);
                        cy = XS_MFMA(ayl, bh[cur], cy);
                        if (j + 4 < 16) { ayh = yfrag(2 * j + 8); ayl = yfrag(2 * j + 9); }
                    }
                    // (a wave-uniform branch, not a third variant of this loop: two more copies of it and the weights no longer stay put
                    // in their registers.  The output head's variant has no register left for the DMA: its phases never issue.)
                    if (!YK && j < XS_PG_NP && issue) {
                        if (STEADY) xs_gather_piece_steady(prws, ylane, gs, j);
                        else xs_gather_piece(prws, ylane, go, j, w);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (YK)
                    (&sHAND[p & 1][w][0] + lane)[128] = make_float4(fmaf(cy[0], XS_ISCALE, my[0]), fmaf(cy[1], XS_ISCALE, my[1]),
                                                                    fmaf(cy[2], XS_ISCALE, my[2]), fmaf(cy[3], XS_ISCALE, my[3]));
            };
            if (ycu) products(std::true_type{});
            else if (YH && ps == T + 2) {     // the extra step of the output head: nothing to compute on the other CUs
                if (issue) {
#pragma unroll
                    for (int j = 0; j < XS_PG_NP; ++j) {
                        if (STEADY) xs_gather_piece_steady(prws, ylane, gs, j);
                        else xs_gather_piece(prws, ylane, go, j, w);
                    }
                }
            } else products(std::false_type{});
            if (mtracer) a.trace[(long)p * 8 + 1] = clock64();
            float4 *hd_ = &sHAND[p & 1][w][0] + lane;
            hd_[0] = make_float4(fmaf(c2[0], XS_ISCALE, m2[0]), fmaf(c2[1], XS_ISCALE, m2[1]), fmaf(c2[2], XS_ISCALE, m2[2]), fmaf(c2[3], XS_ISCALE, m2[3]));
            hd_[64] = make_float4(fmaf(c1[0], XS_ISCALE, m1[0]), fmaf(c1[1], XS_ISCALE, m1[1]), fmaf(c1[2], XS_ISCALE, m1[2]), fmaf(c1[3], XS_ISCALE, m1[3]));
            // barrier p (no look at the abort word: see opnet_xcd_forward); behind it the next phase reads what this wave gathered
            if (issue) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            // (stamp 3 is this wave's when the launch gathers from here - the finish wave then leaves it alone; bit 0 = issued)
            if (mtracer && pg) a.trace[(long)p * 8 + 3] = (clock64() & ~1ull) | (issue ? 1ull : 0ull);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (!STEADY && ng == 1) {           // exposed exchange: wait for this phase's finish + the next gather
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
            }
            if (STEADY) pcu += pgi + 1 == ng ? pcu_wrap : 11;
            if (++pgi == ng) { pgi = 0; ++ps; }
        }
        return;
    }

    // ============================================== finish waves ======================================================
    const unsigned NS = STEADY || a.ring ? (unsigned)XCD_RING : (unsigned)(T + 1);
    const unsigned smask = STEADY || a.ring ? (unsigned)(XCD_RING - 1) : 0xffffffffu;
    const unsigned lds0 = (unsigned)(unsigned long long)(const void *)&sbuf[0][0];
    const __amdgpu_buffer_rsrc_t rws = __builtin_amdgcn_make_buffer_rsrc((void *)a.ws, 0, 0x7fffffff, 0x00020000);
    const unsigned lane16 = lane * 16;
    const unsigned xq_voff = ((6 * u) * 16 + n) * 16;            // this lane's first k-quad of the fp32 image of x
    const unsigned flag_voff = (lane & 31) * 4;
    // lanes 0..15 store the hi halfs of clip `lane`'s four units, lanes 16..31 the lo halfs: byte offset inside a tile's block
    const unsigned pl_voff = (u & 1) * 1024 + n * 16;
    unsigned lg_voff[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) lg_voff[r] = (4 * u + r < OPNET_SLOTS_) ? (unsigned)(((n * OPNET_SLOTS_ + 4 * u + r) * T) * 4) : 0xffffffffu;
    bool alive = true;

    // this wave's share (pieces w, w+4, ...) of the gather of phase (group gi, step s) into LDS buffer `buf`:
    // x = pieces 0..5, h1 = 6..21, h2 = 22..53, frames_boxes = 54, 55
    auto gather = [&](int gi, int s, int buf, int w) {
        const XsGather o = xs_gather_of(sa, lds0, g0, NS, smask, gi, s, buf, w);
#pragma unroll
        for (int j = 0; j < XS_CHUNKS / 4; ++j) xs_gather_piece(rws, lane16, o, j, w);
    };
    auto flags_ready = [&](int gn, unsigned need) -> bool {
        const unsigned v = __builtin_amdgcn_raw_buffer_load_b32(rws, flag_voff, a.flags_off + (g0 + gn) * (XCD_CUS * 4), 16);   // sc1
        return __all(v >= need);
    };
    auto poll_gather = [&](int gn, int sn, int buf, int phase, int w, unsigned cf) {
        if (!alive || (cf & XCD_CF_DBG1)) return;
        if (sn > 0 && !flags_ready(gn, (unsigned)sn))
            alive = xcd_wait_flags_ws(rws, a.flags_off + (g0 + gn) * (XCD_CUS * 4), (unsigned)sn, XS_KARG32(status_off), phase);
        if (alive) gather(gn, sn, buf, w);
        else XCD_LDS_ST(sAbort, 1);
    };

    gather(0, 0, 0, w);                         // phase 0 reads only zero slots and x[0]: nothing to wait for
    if (ng >= 2 && nph > 1) gather(1, 0, 1, w);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (XCD_LDS_LD(sAbort)) return;
    const unsigned cfbits = (ng >= 4 ? XCD_CF_NG4 : 0u) | (ng >= 2 ? XCD_CF_NG2 : 0u) | (ng == 1 ? XCD_CF_NG1 : 0u)
                            | ((a.debug & 1) ? XCD_CF_DBG1 : 0u) | ((a.debug & 2) ? XCD_CF_DBG2 : 0u) | ((a.debug & 4) ? XCD_CF_DBG4 : 0u)
                            | ((a.debug & 8) ? XCD_CF_DBG8 : 0u) | (a.ring ? XCD_CF_RING : 0u) | (sa.pgather != 0 && ng >= 4 ? XS_CF_PG : 0u)
                            | (__builtin_amdgcn_readfirstlane(XCD_LDS_LD(sLocal)) != 0 ? XCD_CF_LOCAL : 0u)
                            | ((TRACE && a.trace && blockIdx.x == 0 && wv == XCD_FW0) ? XCD_CF_TRACE : 0u);

    int gi = 0, s = 0;                          // phase fp = s * ng + gi
    // steady: s + 11 gi, carried with the phase - xcd_head_cu(s, gi) = fcu & 31 and xcd_y_cu(s, gi) = (fcu + 16) & 31 without the multiply
    int fcu = 0;
    const int fcu_wrap = 1 - 11 * (ng - 1);
#if XS_ELOOK
    unsigned ev = 0u;                           // wave 0: the flags requested at the end of the phase before (0 passes for no step > 0)
#endif
    for (int fp = 0; fp < nph; ++fp) {
        unsigned cf = __builtin_amdgcn_readfirstlane(cfbits);
        int wq = w;
        asm volatile("" : "+s"(cf), "+s"(wq));
        // steady: only the store form (and, with stamps, the tracer) is a run-time bit - every test of another bit folds away
        if (STEADY) cf = (cf & (XCD_CF_LOCAL | (TRACE ? XCD_CF_TRACE : 0u))) | XCD_CF_NG4 | XCD_CF_NG2 | XCD_CF_RING | XS_CF_PG;
        const bool local = (cf & XCD_CF_LOCAL) != 0, tracer = (cf & XCD_CF_TRACE) != 0 && lane == 0;
        const unsigned gg = g0 + gi;
        const int ahead = (cf & XCD_CF_NG2) ? 2 : 1;
        int gn = gi + ahead, sn = s;
        if (STEADY) { if (gn >= ng) { gn -= ng; ++sn; } }      // ahead = 2 < 4 <= ng: at most one wrap
        else while (gn >= ng) { gn -= ng; ++sn; }
        // the selection head of step s-1: wave 0 of the step's head CU alone.  boxes[s-1] (fp32 image) and the 16 split A fragments
        // of W_sel are requested before the barrier, so that the round trips are over when the phase's sums arrive
        const bool head_cu = (STEADY ? (fcu & (XCD_CUS - 1)) : xcd_head_cu(s, gi)) == c
                             && (STEADY ? (unsigned)(s - 1) < (unsigned)T : (s >= 1 && s <= T));   // (one compare: the compiler keeps two and their masks)
        const bool head_wave = head_cu && wq == 0;
        xcd_u32x4 xq[6];
        xs_h8 wsh[8], wsl[8];
        if (head_wave) {
            const unsigned xs = XS_KARG32(xp_off) + ((gg * (T + 2) + s) * OPNET_KXQ) * 256;
#pragma unroll
            for (int j = 0; j < 6; ++j) xq[j] = __builtin_amdgcn_raw_buffer_load_b128(rws, xq_voff + j * 256, xs, 0);
            const xs_h8 *ps = (const xs_h8 *)((const char *)xcd_karg_u64<(unsigned)__builtin_offsetof(XcdSplitArgs, wsp)>() + P.wselp * 4) + lane;
#pragma unroll
            for (int q = 0; q < 8; ++q) { wsh[q] = ps[(2 * q) * 64]; wsl[q] = ps[(2 * q + 1) * 64]; }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();           // barrier fp: the phase's accumulators are in sHAND[fp & 1]
        asm volatile("" ::: "memory");
        if (tracer) XCD_KARG(unsigned long long *, trace)[(long)fp * 8 + 2] = clock64();
        if (XCD_LDS_LD(sAbort)) return;
        bool early = false;
        if (cf & XS_CF_PG) {
            // the verdict wave 0 posted before this barrier: ready = the product waves issue the gather of phase fp + 2 right now
            early = __builtin_amdgcn_readfirstlane(XCD_LDS_LD(sPG[fp & 1])) != 0;
            if (XS_PG_NP < XS_CHUNKS / 4 && early) {
                const XsGather o = xs_gather_of(sa, lds0, g0, NS, smask, gn, sn, fp & 1, wq);
                if (STEADY) {
                    xs_gather_finish_run(rws, lane16, xs_gather_steady_of(o, wq));
                } else {
#pragma unroll
                    for (int j = XS_PG_NP; j < XS_CHUNKS / 4; ++j) xs_gather_piece(rws, lane16, o, j, wq);
                }
            }
        } else if ((cf & XCD_CF_NG4) && !head_cu && fp + 2 < nph && alive && !(cf & XCD_CF_DBG1) && (sn == 0 || flags_ready(gn, (unsigned)sn))) {
            gather(gn, sn, fp & 1, wq);
            early = true;
        }
        if (tracer && !(cf & XS_CF_PG)) XCD_KARG(unsigned long long *, trace)[(long)fp * 8 + 3] = clock64();

        const float4 *H = &sHAND[fp & 1][0][0] + lane;
        // ---- selection head of step s-1: logits, softmax, einsum -> frames_boxes[s-1], which travels to every CU with this
        //      phase's publish and enters LSTM2 as the 17th block one step later ---------------------------------------------
        if (head_wave && !(alive && !(cf & XCD_CF_DBG2)) && lane == 0) XCD_LDS_ST(sH1done, fp + 1);   // skipped head: still release the buffer
        if (head_wave && alive && !(cf & XCD_CF_DBG2)) {
            float v[4];
            {
                // the whole 16 x 256 x 16-clip product on this one wave: B fragments = h1[s-1] out of the phase's gather buffer
                // (which the gather of the phase after next will overwrite: sH1done releases it)
                const xs_h8 *Fh = &sbuf[fp & 1][XS_H1] + lane;
                xs_h8 bh[8], bl[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) { bh[q] = Fh[(2 * q) * 64]; bl[q] = Fh[(2 * q + 1) * 64]; }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (lane == 0) XCD_LDS_ST(sH1done, fp + 1);
                f32x4 hm = {0.f, 0.f, 0.f, 0.f}, hc = hm;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    hm = XS_MFMA(wsh[q], bh[q], hm);
                    hc = XS_MFMA(wsh[q], bl[q], hc);
                    hc = XS_MFMA(wsl[q], bh[q], hc);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaf(hc[r], XS_ISCALE, hm[r]);
            }
            {
                float *lg = XCD_KARG(float *, logits) + ((long)gg * 16 * OPNET_SLOTS_) * T + (s - 1);
                const bool clip_ok = (int)(gg * 16 + n) < (int)XS_KARG32(B);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (clip_ok && lg_voff[r] != 0xffffffffu) *(float *)((char *)lg + lg_voff[r]) = v[r];
            }
            float m = fmaxf(fmaxf(v[0], v[1]), v[2]);
            if (u < 3) m = fmaxf(m, v[3]);                        // slot 15 does not exist
            m = fmaxf(m, __shfl_xor(m, 16));
            m = fmaxf(m, __shfl_xor(m, 32));
            float e[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) e[r] = __expf(v[r] - m);
            if (u == 3) e[3] = 0.f;
            float sum = (e[0] + e[1]) + (e[2] + e[3]);
            sum += __shfl_xor(sum, 16);
            sum += __shfl_xor(sum, 32);
            const float inv = __builtin_amdgcn_rcpf(sum);
            const float pr[4] = {e[0] * inv, e[1] * inv, e[2] * inv, e[3] * inv};
            const float xf[24] = {__uint_as_float(xq[0].x), __uint_as_float(xq[0].y), __uint_as_float(xq[0].z), __uint_as_float(xq[0].w),
                                  __uint_as_float(xq[1].x), __uint_as_float(xq[1].y), __uint_as_float(xq[1].z), __uint_as_float(xq[1].w),
                                  __uint_as_float(xq[2].x), __uint_as_float(xq[2].y), __uint_as_float(xq[2].z), __uint_as_float(xq[2].w),
                                  __uint_as_float(xq[3].x), __uint_as_float(xq[3].y), __uint_as_float(xq[3].z), __uint_as_float(xq[3].w),
                                  __uint_as_float(xq[4].x), __uint_as_float(xq[4].y), __uint_as_float(xq[4].z), __uint_as_float(xq[4].w),
                                  __uint_as_float(xq[5].x), __uint_as_float(xq[5].y), __uint_as_float(xq[5].z), __uint_as_float(xq[5].w)};
            xs_h8 fh = (xs_h8)(_Float16)0, fl = fh;
#pragma unroll
            for (int f = 0; f < OPNET_FEATS_; ++f) {
                float t = pr[0] * xf[f];
                t = fmaf(pr[1], xf[6 + f], t);
                t = fmaf(pr[2], xf[12 + f], t);
                t = fmaf(pr[3], xf[18 + f], t);
                t += __shfl_xor(t, 16);
                t += __shfl_xor(t, 32);
                _Float16 h, q;
                xs_split(t, &h, &q);
                fh[f] = h; fl[f] = q;
            }
            // every lane now holds the clip's six values: lanes 0..15 store the hi halfs (k = 0..7, 6 and 7 zero) of clip `lane`,
            // lanes 16..31 the lo halfs, of slot s (= frames_boxes[s-1])
            if (lane < 32) {
                const unsigned fo = a.fb_off + (gg * NS + ((unsigned)s & smask)) * 2048;
                const xcd_u32x4 pv = __builtin_bit_cast(xcd_u32x4, u == 0 ? fh : fl);
                if (local) __builtin_amdgcn_raw_buffer_store_b128(pv, rws, pl_voff, fo, 0);
                else __builtin_amdgcn_raw_buffer_store_b128(pv, rws, pl_voff, fo, 16);
            }
        }
        if (tracer) XCD_KARG(unsigned long long *, trace)[(long)fp * 8 + 4] = clock64();
        // ---- LSTM2 cell of step s-2: lane (clip n, unit 4 t2 + u); the gates arrive complete ----------------------------------
        if ((STEADY ? (unsigned)(s - 2) < (unsigned)T : (s >= 2 && s <= T + 1)) && alive && !(cf & XCD_CF_DBG4)) {
            const float4 g2 = H[w * XH_F4];
            float cc = sC2[gi][w][lane];
            const float h = lstm_cell(g2.x, g2.y, g2.z, g2.w, &cc);
            sC2[gi][w][lane] = cc;
            _Float16 hh, hl;
            xs_split(h, &hh, &hl);
            sTR[w][0][0][n * 4 + u] = hh;
            sTR[w][0][1][n * 4 + u] = hl;
            XCD_WAVE_LDS_SYNC();
            if (lane < 32) {
                // units 4 t2 .. 4 t2 + 3 = k: block t2 >> 3, lane group (t2 & 7) >> 1, halfs 4 (t2 & 1) ..
                const xs_u32x2 hv = *(const xs_u32x2 *)&sTR[w][0][u & 1][n * 4];
                xs_store8(rws, pl_voff, a.h2_off + ((gg * NS + ((unsigned)(s - 1) & smask)) * (XCD_H2 / 4)) * 256
                                            + (t2 >> 3) * 2048 + ((t2 & 7) >> 1) * 256 + (t2 & 1) * 8, hv, local);
            }
        }
        // ---- LSTM1 cell of step s, by the upper-K wave of each pair --------------------------------------------------------
        if ((wq & 1) && s < T && alive && !(cf & XCD_CF_DBG4)) {
            const float4 lo = H[(w - 1) * XH_F4 + 64], hi = H[w * XH_F4 + 64];
            float cc = sC1[gi][w >> 1][lane];
            const float h = lstm_cell(lo.x + hi.x, lo.y + hi.y, lo.z + hi.z, lo.w + hi.w, &cc);
            sC1[gi][w >> 1][lane] = cc;
            _Float16 hh, hl;
            xs_split(h, &hh, &hl);
            sTR[w][1][0][n * 4 + u] = hh;
            sTR[w][1][1][n * 4 + u] = hl;
            XCD_WAVE_LDS_SYNC();
            if (lane < 32) {
                const xs_u32x2 hv = *(const xs_u32x2 *)&sTR[w][1][u & 1][n * 4];
                xs_store8(rws, pl_voff, a.h1_off + ((gg * NS + ((unsigned)(s + 1) & smask)) * (XCD_H1 / 4)) * 256
                                            + (t1 >> 3) * 2048 + ((t1 & 7) >> 1) * 256 + (t1 & 1) * 8, hv, local);
            }
        }
        if (tracer) XCD_KARG(unsigned long long *, trace)[(long)fp * 8 + 5] = clock64();
        // ---- publish: every finish wave drains its stores (and DMA) and arrives at an LDS counter; the last one stores the
        //      CU's flag -------------------------------------------------------------------------------------------------------
#if XS_ELOOK
        // (ev is an operand so that its first use - and with it a wait for the early look - cannot be scheduled ahead of this wait)
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(ev) :: "memory");
#else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        if (alive && !(cf & XCD_CF_DBG8)) {
            const bool last = (xcd_lds_add_lane0((unsigned)(unsigned long long)(const void *)&sArrive[fp & 1], 1u) & 3u) == 3u;
            if (last && lane == 0) {
                if (local) __builtin_amdgcn_raw_buffer_store_b32((unsigned)(s + 1), rws, 0, a.flags_off + (gg * XCD_CUS + c) * 4, 0);
                else __builtin_amdgcn_raw_buffer_store_b32((unsigned)(s + 1), rws, 0, a.flags_off + (gg * XCD_CUS + c) * 4, 16);
            }
        }
        if ((cf & XCD_CF_RING) && wq == 2 && s >= 3 && (STEADY ? ((fcu + 16) & (XCD_CUS - 1)) : xcd_y_cu(s, gi)) == c && alive && !(cf & XCD_CF_DBG4)) {
            // output head of step s-3: the four product waves' K quarters in wave order; rows 0..3 = lanes 0..15 (clip = lane)
            const float4 p0 = H[0 * XH_F4 + 128], p1 = H[1 * XH_F4 + 128], p2 = H[2 * XH_F4 + 128], p3 = H[3 * XH_F4 + 128];
            const long b = (long)gg * 16 + lane;
            if (lane < 16 && b < (long)(int)XS_KARG32(B))
                XCD_KARG(float4 *, y)[b * T + (s - 3)] = make_float4(((p0.x + p1.x) + p2.x) + p3.x, ((p0.y + p1.y) + p2.y) + p3.y,
                                                               ((p0.z + p1.z) + p2.z) + p3.z, ((p0.w + p1.w) + p2.w) + p3.w);
        }
        if (tracer) XCD_KARG(unsigned long long *, trace)[(long)fp * 8 + 6] = clock64();
        if (!early && fp + ahead < nph) {
            if (head_cu && (cf & XCD_CF_NG2)) {           // the gather fills the buffer this CU's head wave read h1 from
                while (XCD_LDS_LD(sH1done) < fp + 1 && !XCD_LDS_LD(sAbort)) __builtin_amdgcn_s_sleep(1);
            }
            poll_gather(gn, sn, (fp + ahead) & 1, fp, wq, cf);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        if ((cf & XS_CF_PG) && wq == 0) {
            // The verdict for barrier fp + 1, in the time this wave used to wait for it: is the gather of phase fp + 3 ready?  One look
            // at the 32 flags, never a spin - not ready, and the finish waves poll and gather it themselves at the end of the next
            // phase (above), with the bounded spin and the abort word.  Never ready on the CU whose wave 0 reads h1 for the selection
            // head out of the buffer that gather fills (sH1done), nor where the product waves then compute the output head (that variant of the
            // product loop has no register left: it spills with the DMA in it) - 2 phases in 32 per CU stay with the finish waves.
            int g1 = gi + 1, s1 = s, g2 = gi + 2, s2 = s, g3 = gi + 3, s3 = s;
            if (g1 >= ng) { g1 -= ng; ++s1; }
            if (g2 >= ng) { g2 -= ng; ++s2; }
            if (g3 >= ng) { g3 -= ng; ++s3; }
            // (steady: the carried counter one and two phases on; a wrap of the group adds fcu_wrap instead of 11)
            const int hcu1 = STEADY ? ((fcu + (g1 == 0 ? fcu_wrap : 11)) & (XCD_CUS - 1)) : xcd_head_cu(s1, g1);
            const int ycu2 = STEADY ? ((fcu + (g1 == 0 ? fcu_wrap : 11) + (g2 == 0 ? fcu_wrap : 11) + 16) & (XCD_CUS - 1)) : xcd_y_cu(s2, g2);
            bool ready = fp + 3 < nph && alive && !(cf & XCD_CF_DBG1) && !(hcu1 == c && (STEADY ? (unsigned)(s1 - 1) < (unsigned)T : (s1 >= 1 && s1 <= T)))
                         && !((cf & XCD_CF_RING) && s2 >= 3 && ycu2 == c);
#if XS_ELOOK
            // "ready" is only ever posted from a look that saw all 32 flags, and never less often than with the late look alone
            if (ready && s3 > 0 && !__all(ev >= (unsigned)s3)) ready = flags_ready(g3, (unsigned)s3);
            if (lane == 0) XCD_LDS_ST(sPG[(fp + 1) & 1], ready ? 1 : 0);
            {
                int g4 = g3 + 1;                // the group of the next verdict: always one of this XCD's, whatever the verdict will need
                if (g4 >= ng) g4 = 0;
                ev = __builtin_amdgcn_raw_buffer_load_b32(rws, flag_voff, a.flags_off + (g0 + g4) * (XCD_CUS * 4), 16);   // sc1
            }
#else
            if (ready && s3 > 0) ready = flags_ready(g3, (unsigned)s3);
            if (lane == 0) XCD_LDS_ST(sPG[(fp + 1) & 1], ready ? 1 : 0);
#endif
        }
        if (tracer) XCD_KARG(unsigned long long *, trace)[(long)fp * 8 + 7] = clock64();
        if (cf & XCD_CF_NG1) {
            __syncthreads();
            if (XCD_LDS_LD(sAbort)) return;
        }
        if (STEADY) fcu += gi + 1 == ng ? fcu_wrap : 11;
        if (++gi == ng) { gi = 0; ++s; }
    }
}

// y[b][t][0..3] = W_out h2[t][b] from the split h2 history (full-history layout): h = hi + lo * 2^-11, W_out exact fp32.
// One workgroup per (group, t): thread (r, n) walks k-octets r, r + 16, ... of clip n, the 16 partials are summed in fixed
// order.  An aborted persistent launch (status[0] != 0) poisons y with NaN.
__global__ void __launch_bounds__(256) opnet_xcd_out_head_split(const XcdArgs a, float *__restrict__ y)
{
    __shared__ float sw[4][XCD_H2];
    __shared__ __attribute__((aligned(16))) float4 red[16][16];
    const int t = blockIdx.x, gg = blockIdx.y, tid = threadIdx.x, T = a.T;
    const PackedLayout P = packed_layout(XCD_H1, XCD_H2);
    const float *wo = a.packed + P.woutp;      // [H2/16][64][4]: lane l = row l & 15, k = 16 q + 4 (l >> 4) + e
    for (int i = tid; i < 4 * XCD_H2; i += 256) {
        const int o = i / XCD_H2, k = i % XCD_H2;
        sw[o][k] = wo[(((k >> 4) * 64) + o + 16 * ((k & 15) >> 2)) * 4 + (k & 3)];
    }
    __syncthreads();
    const int r = tid >> 4, n = tid & 15;
    const xs_h8 *h = (const xs_h8 *)(a.h2h + ((long)gg * (T + 1) + t + 1) * (XCD_H2 * 4));
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ko = r; ko < XCD_H2 / 8; ko += 16) {
        // k = 8 ko + j: block ko >> 2, lane group ko & 3
        const xs_h8 *p = h + (ko >> 2) * 128 + (ko & 3) * 16 + n;
        const xs_h8 hi = p[0], lo = p[64];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float hv = fmaf((float)lo[j], XS_ISCALE, (float)hi[j]);
#pragma unroll
            for (int o = 0; o < 4; ++o) acc[o] = fmaf(sw[o][8 * ko + j], hv, acc[o]);
        }
    }
    red[r][n] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    __syncthreads();
    if (tid < 16) {
        float4 sum = red[0][tid];
        for (int i = 1; i < 16; ++i) {
            const float4 v = red[i][tid];
            sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
        }
        const long b = (long)gg * 16 + tid;
        if (a.status[0] != 0u) sum = make_float4(NAN, NAN, NAN, NAN);
        if (b < a.B) ((float4 *)y)[b * T + t] = sum;
    }
}
