// quad_sigma: upstream's Gaussian blur (quad_sigma > 0) or sharpening (< 0) of the decimated image, between the decimation
// and the tile cut.  Off by default: the kernel is only launched after asl_detector_set_quad_sigma (aprilslam.hip).
// The definition is tests/blur_ref.py: separable, taps uint8 = floor(255 * normalised Gaussian), every sum >> 8, and in each
// direction pixel i of n is filtered for r <= i <= n - r - 2 and copied otherwise (r = ksz / 2; the asymmetry is upstream's).
//
// One workgroup per 64 x 16 output pixels.  The pixels plus a halo of r <= 7 go into LDS (2.4 KB), the horizontal pass
// filters the 16 + 2r rows into a second LDS image (1.9 KB), the vertical pass reads that one column-wise.  A thread owns
// 4 consecutive pixels of a row in both passes; lanes l, l+16, l+32, l+48 of a wavefront own the 4 rows of one 4x4
// threshold tile, whose extrema (of the values written, so k_tile_cut cuts on the blurred image) take two shuffles.
// Algorithmic bytes: npix read + npix written + 2 per tile.
#define BLUR_TW 64
#define BLUR_TH 16
#define BLUR_HALO 7                            /* ksz <= 15 */
#define BLUR_ROWS (BLUR_TH + 2 * BLUR_HALO)
#define BLUR_IN_PITCH ((BLUR_TW + 16) / 4)     /* dwords: columns x0 - 8 .. x0 + 71 */
#define BLUR_H_PITCH (BLUR_TW / 4)             /* dwords: columns x0 .. x0 + 63 */

// The taps centred in 15 bytes, byte u = the weight of offset u - 7 (0 outside the kernel), byte 15 = 0: the window of a
// pixel is then the same 16 bytes for every ksz, and a tap dword that is 0 is skipped by a scalar branch.
struct BlurTaps {
    unsigned int k[4];
    int r;        // ksz / 2, 1..7
    int sharpen;  // quad_sigma < 0: 2 * image - blurred, clipped
};

__global__ void __launch_bounds__(256) k_quad_blur(const uint8_t *__restrict__ dgray, Geom g, BlurTaps taps, uint8_t *__restrict__ out,
                                                   uint8_t *__restrict__ tmin, uint8_t *__restrict__ tmax)
{
    __shared__ unsigned int s_in[BLUR_ROWS * BLUR_IN_PITCH];  // row y0 - 7 + i, columns x0 - 8 ..
    __shared__ unsigned int s_h[BLUR_ROWS * BLUR_H_PITCH];    // the horizontal pass's output, same rows
    const int tid = threadIdx.x, fr = blockIdx.z;
    const int x0 = blockIdx.x * BLUR_TW, y0 = blockIdx.y * BLUR_TH;
    const int r = taps.r;
    const int nrows = BLUR_TH + 2 * r, row0 = BLUR_HALO - r;  // LDS rows row0 .. row0 + nrows - 1 are needed
    const uint8_t *src = dgray + (size_t)fr * g.npix;

    // ---- the tile and its halo: columns x0 - r .. x0 + 63 + r as whole dwords.  A dword that lies inside its image row
    // and is aligned in memory is one load; any other is put together from the bytes that exist.  Pixels outside the image
    // stay 0 and are never used: a filtered pixel has its whole window inside the image.
    {
        const int d_lo = (8 - r) >> 2, ncd = ((BLUR_TW + 7 + r) >> 2) - d_lo + 1;
        for (int i = tid; i < nrows * ncd; i += 256) {
            const int row = i / ncd, k = d_lo + (i - row * ncd);
            const int y = y0 - r + row, x = x0 - 8 + 4 * k;
            unsigned int v = 0;
            if (y >= 0 && y < g.sh) {
                const uint8_t *rowp = src + (size_t)y * g.sw;
                if (x >= 0 && x + 3 < g.sw && ((uintptr_t)(rowp + x) & 3) == 0)
                    v = *reinterpret_cast<const unsigned int *>(rowp + x);
                else
                    for (int b = 0; b < 4; b++)
                        if (x + b >= 0 && x + b < g.sw) v |= (unsigned int)rowp[x + b] << (8 * b);
            }
            s_in[(row0 + row) * BLUR_IN_PITCH + k] = v;
        }
    }
    __syncthreads();

    // ---- horizontal pass over the tile's rows and the vertical halo
    for (int i = tid; i < nrows * 16; i += 256) {
        const int row = i >> 4, q = i & 15;
        const int y = y0 - r + row, xs = x0 + 4 * q;
        if (y < 0 || y >= g.sh) continue;
        const unsigned int *w = s_in + (row0 + row) * BLUR_IN_PITCH + q;  // columns xs - 8 .. xs + 11
        const unsigned int win[5] = {w[0], w[1], w[2], w[3], w[4]};
        unsigned int packed = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {  // pixel xs + j: its 16-byte window starts at byte 1 + j of w
            unsigned int acc = 0;
#pragma unroll
            for (int m = 0; m < 4; m++)
                if (taps.k[m]) {
                    const unsigned int px = j == 3 ? win[m + 1] : __builtin_amdgcn_alignbyte(win[m + 1], win[m], 1 + j);
                    acc = __builtin_amdgcn_udot4(px, taps.k[m], acc, false);
                }
            const int x = xs + j;
            const unsigned int v = (x >= r && x <= g.sw - r - 2) ? acc >> 8 : (win[2] >> (8 * j)) & 0xFFu;
            packed |= v << (8 * j);
        }
        s_h[(row0 + row) * BLUR_H_PITCH + q] = packed;
    }
    __syncthreads();

    // ---- vertical pass, sharpening, tile extrema, store
    const int q = tid & 15, ry = tid >> 4;
    const int y = y0 + ry, xs = x0 + 4 * q;
    unsigned int acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < 2 * BLUR_HALO + 1; u++) {  // offset u - 7: LDS row ry + u
        const unsigned int kb = (taps.k[u >> 2] >> (8 * (u & 3))) & 0xFFu;
        if (kb) {
            const unsigned int h = s_h[(ry + u) * BLUR_H_PITCH + q];
#pragma unroll
            for (int j = 0; j < 4; j++) acc[j] += kb * ((h >> (8 * j)) & 0xFFu);
        }
    }
    const unsigned int hc = s_h[(ry + BLUR_HALO) * BLUR_H_PITCH + q];
    const unsigned int orig = s_in[(ry + BLUR_HALO) * BLUR_IN_PITCH + q + 2];
    const bool filtered = y >= r && y <= g.sh - r - 2;
    unsigned int packed = 0, mn = 255u, mx = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        int v = (int)(filtered ? acc[j] >> 8 : (hc >> (8 * j)) & 0xFFu);
        if (taps.sharpen) v = min(255, max(0, 2 * (int)((orig >> (8 * j)) & 0xFFu) - v));
        packed |= (unsigned int)v << (8 * j);
        mn = min(mn, (unsigned int)v);
        mx = max(mx, (unsigned int)v);
    }
    // lanes l, l + 16, l + 32, l + 48: the four rows of one 4x4 tile (a wavefront is rows 4k .. 4k + 3 of the workgroup's tile)
    mn = min(mn, (unsigned int)__shfl_xor((int)mn, 16)); mx = max(mx, (unsigned int)__shfl_xor((int)mx, 16));
    mn = min(mn, (unsigned int)__shfl_xor((int)mn, 32)); mx = max(mx, (unsigned int)__shfl_xor((int)mx, 32));
    const int tx = (x0 >> 2) + q, ty = (y0 >> 2) + (ry >> 2);
    if ((ry & 3) == 0 && tx < g.tw && ty < g.th) {  // full tiles only, as the decimation kernels
        const size_t t = (size_t)fr * g.tw * g.th + (size_t)ty * g.tw + tx;
        tmin[t] = (uint8_t)mn;
        tmax[t] = (uint8_t)mx;
    }
    if (y < g.sh && xs < g.sw) {
        uint8_t *p = out + (size_t)fr * g.npix + (size_t)y * g.sw + xs;
        if (xs + 3 < g.sw && ((uintptr_t)p & 3) == 0)
            *reinterpret_cast<unsigned int *>(p) = packed;
        else
            for (int j = 0; j < 4; j++)
                if (xs + j < g.sw) p[j] = (uint8_t)(packed >> (8 * j));
    }
}
