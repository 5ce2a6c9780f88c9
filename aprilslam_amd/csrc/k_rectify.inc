// The step between calibration and detection, on the device: a frame from a camera with a lens (K, k1 k2 p1 p2 k3) in, the
// gray frame an ideal pinhole K_new would have delivered out (what cv2.undistort / remap do for upstream's users), so a
// calibrated wide-angle camera can feed the batched detector without its frames crossing the bus.  Every output pixel takes
// its centre through K_new^-1, the forward Brown-Conrady model (closed form: no iteration on this side) and K, and samples
// the source bilinearly with the taps clamped to the edge; a BGR tap becomes gray first, with the detector's own formula.
// The arithmetic is that of tests/rectify_ref.py, operation for operation in float64 with contraction off, so the frames
// are byte-identical to the NumPy statement's.
//
// No tile is skipped on the strength of its outline: a lens can throw a tile's corners and edge midpoints out of the
// source and keep its middle inside (k1 > 0 large: only the image centre survives), so every pixel runs the outside test.

struct RectifyCam {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;  // the source camera
    double nfx, nfy, ncx, ncy;                  // the pinhole of the output
    int fill;                                   // value of a pixel whose sample lies outside the source
};

// gray value of source pixel (x, y), both inside the frame
template <int CH>
__device__ __forceinline__ int rectify_tap(const uint8_t *__restrict__ src, int w, int stride, int x, int y)
{
    const uint8_t *p = src + (size_t)y * (size_t)stride + (size_t)CH * (size_t)x;
    if (CH == 1) return p[0];
    if (x + 1 < w) {  // one unaligned dword: B, G, R and the next pixel's B, all inside the row
        unsigned int u;
        __builtin_memcpy(&u, p, 4);
        return bgr_gray(u);
    }
    return bgr_gray((unsigned int)p[0] | ((unsigned int)p[1] << 8) | ((unsigned int)p[2] << 16));  // a row's last pixel
}

// value of output pixel (x, y); yn is the row's normalised coordinate
template <int CH>
__device__ __forceinline__ int rectify_pixel(int x, double yn, const uint8_t *__restrict__ src, int w, int h, int stride, const RectifyCam &cam)
{
    const double xn = (x + 0.5 - cam.ncx) / cam.nfx;
    const double r2 = xn * xn + yn * yn;
    const double rad = 1 + ((cam.k3 * r2 + cam.k2) * r2 + cam.k1) * r2;
    const double xd = xn * rad + 2 * cam.p1 * xn * yn + cam.p2 * (r2 + 2 * xn * xn);
    const double yd = yn * rad + cam.p1 * (r2 + 2 * yn * yn) + 2 * cam.p2 * xn * yn;
    const double u = cam.fx * xd + cam.cx;
    const double v = cam.fy * yd + cam.cy;
    if (!(u >= 0 && u < w && v >= 0 && v < h)) return cam.fill;  // a NaN lands here too
    // render_pixel's sampling: clamp to edge, texel centres at +0.5
    const double bx = u - 0.5, by = v - 0.5;
    const double fx0 = floor(bx), fy0 = floor(by);
    const double fx = bx - fx0, fy = by - fy0;
    const int ix = (int)fx0, iy = (int)fy0;  // in [-1, w - 1] x [-1, h - 1]
    const int x0c = min(max(ix, 0), w - 1), x1c = min(max(ix + 1, 0), w - 1), y0c = min(max(iy, 0), h - 1), y1c = min(max(iy + 1, 0), h - 1);
    const double t00 = rectify_tap<CH>(src, w, stride, x0c, y0c), t01 = rectify_tap<CH>(src, w, stride, x1c, y0c);
    const double t10 = rectify_tap<CH>(src, w, stride, x0c, y1c), t11 = rectify_tap<CH>(src, w, stride, x1c, y1c);
    const double o = t00 * (1 - fx) * (1 - fy) + t01 * fx * (1 - fy) + t10 * (1 - fx) * fy + t11 * fx * fy;
    double r = floor(o + 0.5);
    r = r < 0 ? 0 : (r > 255 ? 255 : r);
    return (int)r;
}

// One wavefront per 32 x 8 output tile, four consecutive pixels (one dword of gray) per lane, frames along blockIdx.z: the
// shape of k_render.  The taps are plain global loads: neighbouring lanes read neighbouring source bytes, so the gather is
// served by L2; no LDS, no table of precomputed coordinates.
#define RECTIFY_PX 4
#define RECTIFY_TW 32
#define RECTIFY_TH 8
template <int CH>
__global__ void __launch_bounds__(256) k_rectify(const uint8_t *__restrict__ src, int w, int h, int stride, size_t frame_pitch, uint8_t *__restrict__ dst,
                                                 int w_out, int h_out, int stride_out, size_t frame_pitch_out, RectifyCam cam)
{
    const int fr = blockIdx.z;
    const int tx0 = blockIdx.x * RECTIFY_TW;
    const int ty0 = __builtin_amdgcn_readfirstlane((int)((blockIdx.y * 4 + threadIdx.y) * RECTIFY_TH));
    if (ty0 >= h_out) return;
    const int lane = threadIdx.x;
    const int x = tx0 + RECTIFY_PX * (lane & 7), y = ty0 + (lane >> 3);
    if (x >= w_out || y >= h_out) return;
    const uint8_t *s = src + (size_t)fr * frame_pitch;
    const double yn = (y + 0.5 - cam.ncy) / cam.nfy;
    unsigned int val[RECTIFY_PX];
#pragma unroll
    for (int j = 0; j < RECTIFY_PX; j++) val[j] = x + j < w_out ? (unsigned int)rectify_pixel<CH>(x + j, yn, s, w, h, stride, cam) : 0u;
    uint8_t *p = dst + (size_t)fr * frame_pitch_out + (size_t)y * (size_t)stride_out + (size_t)x;
    if (x + RECTIFY_PX <= w_out && ((reinterpret_cast<uintptr_t>(p) & 3u) == 0)) {
        *reinterpret_cast<unsigned int *>(p) = val[0] | (val[1] << 8) | (val[2] << 16) | (val[3] << 24);
    } else {
        for (int j = 0; j < RECTIFY_PX && x + j < w_out; j++) p[j] = (uint8_t)val[j];
    }
}
