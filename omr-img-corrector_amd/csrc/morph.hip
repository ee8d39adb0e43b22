// morph.hip -- erode / dilate with any structuring element getStructuringElement can make (transfer.rs:206-277:
// shape, size, anchor, iterations; BORDER_CONSTANT with morphologyDefaultBorderValue, so positions outside the
// image never take part).  All kernels work on the image as a matrix of BYTES, `wbytes = cols * channels` wide:
// min and max act per byte and a shift of d pixels is a shift of d * channels bytes, which keeps a byte on its
// channel and leaves the row exactly when the pixel leaves the image.  Every lane makes four consecutive bytes.
//
//   morph_spans_lds_kernel     elements up to 31 x 31 as row spans (every shape's rows are one run [j1, j1 + len)):
//                              tile + halo of all fused passes in LDS as dwords, passes ping-pong between two LDS
//                              buffers, positions outside the IMAGE are reset to the neutral value between passes
//                              (the halo of a tile at the image's edge must not carry a minimum of pass p into
//                              pass p + 1 from outside: cv::erode called p times never sees such a value)
//   morph_rect_kernel          full rectangles up to 31 x 31: windows by doubling in LDS -- m_{t+1}(b) =
//                              min(m_t(b), m_t(b + 2^t)), the window of k is min(m_p(b), m_p(b + k - 2^p)) -- along
//                              the rows, then down the columns: log2(kw) + log2(kh) + 2 steps whatever the area
//   morph_spans_global_kernel  everything larger: one byte per lane, a loop over the spans in global memory
//
// The bytewise minimum of two dwords has no instruction on gfx950 (v_pk_min_u16 / v_pk_max_u16 are the narrowest
// packed forms): a dword is split into its even and its odd bytes as two zero-extended u16 pairs -- v_perm_b32
// does the split and the unaligned byte shift in one instruction -- and each half takes one packed op.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace omr {
namespace {

constexpr int MQ = 64;  // output dword columns of a tile (256 bytes)
constexpr int MH = 32;  // output rows of a tile
constexpr size_t MORPH_LDS_MAX = 64 * 1024;

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

template <bool DIL>
__device__ __forceinline__ uint32_t pk(uint32_t a, uint32_t b)
{
    const us2 x = __builtin_bit_cast(us2, a), y = __builtin_bit_cast(us2, b);
    return __builtin_bit_cast(uint32_t, DIL ? __builtin_elementwise_max(x, y) : __builtin_elementwise_min(x, y));
}

// the even (E) and odd (O) bytes of the four bytes that start `o` (0..3) bytes into the pair (lo, hi)
__device__ __forceinline__ void split(uint32_t lo, uint32_t hi, int o, uint32_t *E, uint32_t *O)
{
    *E = __builtin_amdgcn_perm(hi, lo, 0x0c020c00u + (uint32_t)o * 0x00010001u);
    *O = __builtin_amdgcn_perm(hi, lo, 0x0c030c01u + (uint32_t)o * 0x00010001u);
}

struct Img {  // one image of the launch (blockIdx.z)
    const uint8_t *src;
    uint8_t *dst;
    bool src_al, dst_al;  // dword loads / stores allowed
};

__device__ __forceinline__ Img image_of(const MorphImg &im)
{
    Img g;
    g.src = im.src + (int64_t)blockIdx.z * im.sstride;
    g.dst = im.dst + (int64_t)blockIdx.z * im.dstride;
    g.src_al = (((uintptr_t)g.src | (uintptr_t)im.sstep) & 3) == 0;
    g.dst_al = (((uintptr_t)g.dst | (uintptr_t)im.dstep) & 3) == 0;
    return g;
}

// the dword at image row gy, byte column gb (a multiple of 4, possibly negative); neutral outside the image
template <bool DIL>
__device__ __forceinline__ uint32_t load_dword(const Img &g, const MorphImg &im, int gy, int gb)
{
    uint32_t v = DIL ? 0u : 0xffffffffu;
    if ((unsigned)gy >= (unsigned)im.rows || gb < 0 || gb >= im.wbytes) return v;
    const uint8_t *S = g.src + (int64_t)gy * im.sstep + gb;
    if (g.src_al && gb + 4 <= im.wbytes) return *(const uint32_t *)S;
    for (int j = 0; j < 4 && gb + j < im.wbytes; j++) v = (v & ~(255u << (8 * j))) | ((uint32_t)S[j] << (8 * j));
    return v;
}

// the bytes of that dword which lie inside the image
__device__ __forceinline__ uint32_t inside_mask(const MorphImg &im, int gy, int gb)
{
    if ((unsigned)gy >= (unsigned)im.rows || gb < 0 || gb >= im.wbytes) return 0u;
    const int n = im.wbytes - gb;
    return n >= 4 ? 0xffffffffu : (1u << (8 * n)) - 1u;
}

__device__ __forceinline__ void store_dword(const Img &g, const MorphImg &im, int gy, int gb, uint32_t v)
{
    if (gy >= im.rows || gb >= im.wbytes) return;
    uint8_t *D = g.dst + (int64_t)gy * im.dstep + gb;
    if (g.dst_al && gb + 4 <= im.wbytes) {
        *(uint32_t *)D = v;
    } else {
        for (int j = 0; j < 4 && gb + j < im.wbytes; j++) D[j] = (uint8_t)(v >> (8 * j));
    }
}

// tile rows x (ls dwords) from image row ty0, byte column tb0 (a multiple of 4)
template <bool DIL>
__device__ __forceinline__ void stage(uint32_t *t, int lh, int ls, const Img &g, const MorphImg &im, int ty0, int tb0)
{
    for (int i = threadIdx.x; i < lh * ls; i += 256) {
        const int ly = i / ls, lq = i - ly * ls;
        t[i] = load_dword<DIL>(g, im, ty0 + ly, tb0 + 4 * lq);
    }
}

// ------------------------------------------------------------------------------------------
// Row spans in LDS.  A pass needs hl dwords to the left and hr to the right of a dword it makes (the element's
// reach in bytes, rounded up), `top` rows above and `bot` below; the tile carries `passes` times that around its
// MQ x MH outputs.  Every pass makes all dwords whose taps lie inside the tile; the ones near the tile's rim are
// computed from stale neighbours, and that rim grows by one reach per pass without getting to the outputs.
template <bool DIL>
__global__ __launch_bounds__(256) void morph_spans_lds_kernel(MorphImg im, MorphSpans sp, int kh, int ax, int ay, int hl,
                                                              int hr, int passes)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t morph_lds[];
    const Img g = image_of(im);
    const int top = ay, bot = kh - 1 - ay, cn = im.cn;
    const int lq = passes * (hl + hr) + MQ, ls = lq + 1;  // + 1: the pair's second dword of the rightmost tap
    const int lh = passes * (top + bot) + MH;
    const int ty0 = blockIdx.y * MH - passes * top, tb0 = (blockIdx.x * MQ - passes * hl) * 4;
    uint32_t *b0 = morph_lds, *b1 = morph_lds + lh * ls;
    stage<DIL>(b0, lh, ls, g, im, ty0, tb0);
    __syncthreads();
    for (int pass = 1; pass <= passes; pass++) {
        const uint32_t *A = (pass & 1) ? b0 : b1;
        uint32_t *B = (pass & 1) ? b1 : b0;
        const bool last = pass == passes;
        const int r0 = last ? passes * top : top, q0 = last ? passes * hl : hl;
        const int h = last ? MH : lh - top - bot, w = last ? MQ : lq - hl - hr;
        for (int idx = threadIdx.x; idx < w * h; idx += 256) {
            const int r = r0 + idx / w, q = q0 + idx % w;
            uint32_t aE = DIL ? 0u : 0x00ff00ffu, aO = aE;
            for (int i = 0; i < kh; i++) {
                const int len = sp.len[i];
                const uint32_t *row = A + (r + i - ay) * ls + q;
                int d = ((int)sp.j1[i] - ax) * cn, cur = -(1 << 30);
                uint32_t lo = 0, hi = 0;
                for (int t = 0; t < len; t++, d += cn) {
                    const int dq = d >> 2;
                    if (dq != cur) {  // uniform: d does not depend on the lane
                        lo = dq == cur + 1 ? hi : row[dq];
                        hi = row[dq + 1];
                        cur = dq;
                    }
                    uint32_t E, O;
                    split(lo, hi, d & 3, &E, &O);
                    aE = pk<DIL>(aE, E);
                    aO = pk<DIL>(aO, O);
                }
            }
            const uint32_t v = aE | (aO << 8);
            const int gy = ty0 + r, gb = tb0 + 4 * q;
            if (last) {
                store_dword(g, im, gy, gb, v);
            } else {
                const uint32_t in = inside_mask(im, gy, gb);
                B[r * ls + q] = DIL ? (v & in) : (v | ~in);
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// Full rectangle kw x kh (both <= MORPH_MAXK), anchor (ax, ay).  Tile rows: MH + kh - 1 from row -ay; tile dwords:
// `ls` (the host's morph_rect_ls: the outputs, the window's reach and one dword per step for the rounding of the
// byte shifts to dwords) from the dword that holds byte -ax * cn of the first output.
template <bool DIL>
__device__ __forceinline__ uint32_t min2_shifted(const uint32_t *row, int off0, int off1)
{
    uint32_t E0, O0, E1, O1;
    split(row[off0 >> 2], row[(off0 >> 2) + 1], off0 & 3, &E0, &O0);
    split(row[off1 >> 2], row[(off1 >> 2) + 1], off1 & 3, &E1, &O1);
    return pk<DIL>(E0, E1) | (pk<DIL>(O0, O1) << 8);
}

template <bool DIL>
__device__ __forceinline__ uint32_t min2(uint32_t a, uint32_t b)
{
    return pk<DIL>(a & 0x00ff00ffu, b & 0x00ff00ffu) | (pk<DIL>((a >> 8) & 0x00ff00ffu, (b >> 8) & 0x00ff00ffu) << 8);
}

template <bool DIL>
__global__ __launch_bounds__(256) void morph_rect_kernel(MorphImg im, int kw, int kh, int ax, int ay, int ls)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t morph_lds[];
    const Img g = image_of(im);
    const int cn = im.cn, lh = MH + kh - 1;
    const int ql = (ax * cn + 3) >> 2, e = 4 * ql - ax * cn;  // the first output's window starts e bytes into dword 0
    const int ty0 = blockIdx.y * MH - ay, tb0 = (blockIdx.x * MQ - ql) * 4;
    uint32_t *A = morph_lds, *B = morph_lds + lh * ls;
    stage<DIL>(A, lh, ls, g, im, ty0, tb0);
    __syncthreads();
    // along the rows: valid dwords [0, v) shrink by the shift and the pair's second dword each step
    int v = ls, span = 1;
    while (2 * span <= kw) {
        const int s = span * cn;
        v -= (s >> 2) + 1;
        for (int idx = threadIdx.x; idx < lh * v; idx += 256) {
            const int r = idx / v, q = idx - r * v;
            B[r * ls + q] = min2_shifted<DIL>(A + r * ls + q, 0, s);
        }
        __syncthreads();
        uint32_t *t = A;
        A = B, B = t, span *= 2;
    }
    for (int idx = threadIdx.x; idx < lh * MQ; idx += 256) {
        const int r = idx / MQ, q = idx - r * MQ;
        B[r * ls + q] = min2_shifted<DIL>(A + r * ls + q, e, e + (kw - span) * cn);
    }
    __syncthreads();
    {
        uint32_t *t = A;
        A = B, B = t;
    }
    // down the columns (dwords stay aligned)
    int vr = lh;
    span = 1;
    while (2 * span <= kh) {
        vr -= span;
        for (int idx = threadIdx.x; idx < vr * MQ; idx += 256) {
            const int r = idx / MQ, q = idx - r * MQ;
            B[r * ls + q] = min2<DIL>(A[r * ls + q], A[(r + span) * ls + q]);
        }
        __syncthreads();
        uint32_t *t = A;
        A = B, B = t, span *= 2;
    }
    for (int idx = threadIdx.x; idx < MH * MQ; idx += 256) {
        const int r = idx / MQ, q = idx - r * MQ;
        store_dword(g, im, blockIdx.y * MH + r, (blockIdx.x * MQ + q) * 4,
                    min2<DIL>(A[r * ls + q], A[(r + kh - span) * ls + q]));
    }
}

// ------------------------------------------------------------------------------------------
// Any size: one byte per lane, the spans (d_spans: kh pairs j1, len) walked in global memory, both loops clamped
// to the image so that an element far larger than the image costs what the image costs.
template <bool DIL>
__global__ __launch_bounds__(256) void morph_spans_global_kernel(MorphImg im, const int32_t *__restrict__ d_spans, int kh,
                                                                 int ax, int ay)
{
    const int b = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (b >= im.wbytes) return;
    const uint8_t *S = im.src + (int64_t)blockIdx.z * im.sstride;
    const int cn = im.cn, x = b / cn, cols = im.wbytes / cn;
    int acc = DIL ? 0 : 255;
    const int i0 = max(0, ay - y), i1 = (int)min((int64_t)kh, (int64_t)ay + im.rows - y);
    for (int i = i0; i < i1; i++) {
        const uint8_t *row = S + (int64_t)(y + i - ay) * im.sstep + b;
        const int j0 = max(d_spans[2 * i], ax - x);
        const int j1 = (int)min((int64_t)d_spans[2 * i] + d_spans[2 * i + 1], (int64_t)ax + cols - x);
        for (int j = j0; j < j1; j++) {
            const int p = row[(int64_t)(j - ax) * cn];
            acc = DIL ? max(acc, p) : min(acc, p);
        }
    }
    im.dst[(int64_t)blockIdx.z * im.dstride + (int64_t)y * im.dstep + b] = (uint8_t)acc;
}

dim3 tile_grid(const MorphImg &im)
{
    return dim3((im.wbytes + 4 * MQ - 1) / (4 * MQ), (im.rows + MH - 1) / MH, im.n);
}

size_t spans_lds_bytes(int kh, int hl, int hr, int passes)
{
    const size_t ls = (size_t)passes * (hl + hr) + MQ + 1, lh = (size_t)passes * (kh - 1) + MH;
    return (passes > 1 ? 2 : 1) * lh * ls * sizeof(uint32_t);
}

}  // namespace

int morph_spans_lds_max_passes(int kw, int kh, int ax, int cn)
{
    if (kw > MORPH_MAXK || kh > MORPH_MAXK) return 0;
    const int hl = (ax * cn + 3) / 4, hr = ((kw - 1 - ax) * cn + 3) / 4;
    int f = 1;  // one pass of a 31 x 31 element on 4 channels takes 24 KB
    while ((f + 1) * (kh - 1) <= MH && (f + 1) * (hl + hr) <= MQ / 2 && spans_lds_bytes(kh, hl, hr, f + 1) <= MORPH_LDS_MAX) f++;
    return f;
}

hipError_t launch_morph_spans_lds(const MorphImg &im, int op, const MorphSpans &sp, int kw, int kh, int ax, int ay,
                                  int passes, hipStream_t s)
{
    if (passes < 1 || passes > morph_spans_lds_max_passes(kw, kh, ax, im.cn)) return hipErrorInvalidValue;
    const int hl = (ax * im.cn + 3) / 4, hr = ((kw - 1 - ax) * im.cn + 3) / 4;
    const size_t lds = spans_lds_bytes(kh, hl, hr, passes);
    if (op) hipLaunchKernelGGL(morph_spans_lds_kernel<true>, tile_grid(im), dim3(256), lds, s, im, sp, kh, ax, ay, hl, hr, passes);
    else hipLaunchKernelGGL(morph_spans_lds_kernel<false>, tile_grid(im), dim3(256), lds, s, im, sp, kh, ax, ay, hl, hr, passes);
    return hipGetLastError();
}

hipError_t launch_morph_rect(const MorphImg &im, int op, int kw, int kh, int ax, int ay, hipStream_t s)
{
    if (kw < 1 || kh < 1 || kw > MORPH_MAXK || kh > MORPH_MAXK) return hipErrorInvalidValue;
    const int cn = im.cn, ql = (ax * cn + 3) / 4, e = 4 * ql - ax * cn;
    int span = 1, steps = 0;
    for (; 2 * span <= kw; span *= 2) steps += ((span * cn) >> 2) + 1;
    const int ls = MQ + ((e + (kw - span) * cn) >> 2) + 2 + steps;
    const size_t lds = (size_t)2 * (MH + kh - 1) * ls * sizeof(uint32_t);  // <= 50 KB
    if (op) hipLaunchKernelGGL(morph_rect_kernel<true>, tile_grid(im), dim3(256), lds, s, im, kw, kh, ax, ay, ls);
    else hipLaunchKernelGGL(morph_rect_kernel<false>, tile_grid(im), dim3(256), lds, s, im, kw, kh, ax, ay, ls);
    return hipGetLastError();
}

hipError_t launch_morph_spans_global(const MorphImg &im, int op, const int32_t *d_spans, int kh, int ax, int ay,
                                     hipStream_t s)
{
    const dim3 grid((im.wbytes + 255) / 256, im.rows, im.n);
    if (op) hipLaunchKernelGGL(morph_spans_global_kernel<true>, grid, dim3(256), 0, s, im, d_spans, kh, ax, ay);
    else hipLaunchKernelGGL(morph_spans_global_kernel<false>, grid, dim3(256), 0, s, im, d_spans, kh, ax, ay);
    return hipGetLastError();
}

}  // namespace omr
