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

// the sample of the source at (u, v): `fill` outside the frame, else bilinear with the taps clamped to the edge
template <int CH>
__device__ __forceinline__ int rectify_sample(double u, double v, const uint8_t *__restrict__ src, int w, int h, int stride, int fill)
{
    if (!(u >= 0 && u < w && v >= 0 && v < h)) return fill;  // a NaN lands here too
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

// the forward Brown-Conrady model, closed form: normalised coordinates (xn, yn) -> source pixel coordinates (u, v)
__device__ __forceinline__ void rectify_brown(double xn, double yn, double fx, double fy, double cx, double cy, double k1, double k2, double p1,
                                              double p2, double k3, double &u, double &v)
{
    const double r2 = xn * xn + yn * yn;
    const double rad = 1 + ((k3 * r2 + k2) * r2 + k1) * r2;
    const double xd = xn * rad + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn);
    const double yd = yn * rad + p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn;
    u = fx * xd + cx;
    v = fy * yd + cy;
}

// value of output pixel (x, y); yn is the row's normalised coordinate
template <int CH>
__device__ __forceinline__ int rectify_pixel(int x, double yn, const uint8_t *__restrict__ src, int w, int h, int stride, const RectifyCam &cam)
{
    const double xn = (x + 0.5 - cam.ncx) / cam.nfx;
    double u, v;
    rectify_brown(xn, yn, cam.fx, cam.fy, cam.cx, cam.cy, cam.k1, cam.k2, cam.p1, cam.p2, cam.k3, u, v);
    return rectify_sample<CH>(u, v, src, w, h, stride, cam.fill);
}

// One wavefront per 32 x 8 output tile, four consecutive pixels (one dword of gray) per lane, frames along blockIdx.z: the
// shape of k_render.  The taps are plain global loads: neighbouring lanes read neighbouring source bytes, so the gather is
// served by L2; no LDS, no table of precomputed coordinates.
#define RECTIFY_PX 4
#define RECTIFY_TW 32
#define RECTIFY_TH 8
// a lane's four pixels, the first at column x, to p: one dword where all four are inside the row and p is aligned, bytes otherwise
__device__ __forceinline__ void rectify_store(uint8_t *__restrict__ p, const unsigned int (&val)[RECTIFY_PX], int x, int w_out)
{
    if (x + RECTIFY_PX <= w_out && ((reinterpret_cast<uintptr_t>(p) & 3u) == 0)) {
        *reinterpret_cast<unsigned int *>(p) = val[0] | (val[1] << 8) | (val[2] << 16) | (val[3] << 24);
    } else {
        for (int j = 0; j < RECTIFY_PX && x + j < w_out; j++) p[j] = (uint8_t)val[j];
    }
}

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
    rectify_store(dst + (size_t)fr * frame_pitch_out + (size_t)y * (size_t)stride_out + (size_t)x, val, x, w_out);
}

// ---- rectification into rotated pinhole views: the same tile, blockIdx.z over view * n_frames + frame.  A fisheye of
// 150-200 degrees does not fit one pinhole; it fits a fan of them (left, front, right), and those are a rig of pinhole cameras
// whose mountings are known exactly.  Output pixel (x, y) of view (K_new, R), R = source camera <- view: the view ray
// ((x + 0.5 - cx') / fx', (y + 0.5 - cy') / fy', 1) through R, then the lens, then rectify_sample.  The arithmetic is that of
// tests/rectify_views_ref.py, operation for operation in float64 with contraction off.  All views of a call go in one
// launch chain, so a source frame comes from HBM once and serves the other views out of L2.
#define RECTIFY_LENS_BROWN 0
#define RECTIFY_LENS_FISHEYE 1
#define RECTIFY_MAX_VIEWS 16
struct RectifyView {
    double nfx, nfy, ncx, ncy;  // the pinhole of the view
    double R[9];                // source camera <- view, row-major
};
// by value in the kernel arguments (16 x 104 bytes): no staging copy that a second call could overwrite under the first
struct RectifyViewTable { RectifyView v[RECTIFY_MAX_VIEWS]; };
struct RectifyLens {
    double fx, fy, cx, cy;  // the source camera
    double k[5];            // Brown: k1 k2 p1 p2 k3; fisheye: k1 k2 k3 k4
    double theta_max;       // fisheye: rays further from the axis give `fill`
    int fill;
};

// atan2(r, Z) for r >= 0, in [0, pi]: atan2_pos of the statement.  The device library's atan2 is as good and is another
// function; the frames are defined by this one.  fdlibm's reduction: t = r / |Z| to |x| <= 7/16 around 0, 0.5, 1, 1.5 or inf.
__device__ __forceinline__ double rectify_atan2_pos(double r, double Z)
{
    const double a = Z < 0 ? -Z : Z;
    const double q = r / a;
    const double t = r == 0 ? 0.0 : q;
    const bool c1 = t < 0.4375, c2 = t < 0.6875, c3 = t < 1.1875, c4 = t < 2.4375;
    // the one quotient of the statement's five that is used; t / 1 is t
    const double num = c1 ? t : (c2 ? 2.0 * t - 1.0 : (c3 ? t - 1.0 : (c4 ? t - 1.5 : -1.0)));
    const double den = c1 ? 1.0 : (c2 ? 2.0 + t : (c3 ? t + 1.0 : (c4 ? 1.0 + 1.5 * t : t)));
    const double x = num / den;
    const double hi = c1 ? 0.0 : (c2 ? 4.63647609000806093515e-01 : (c3 ? 7.85398163397448278999e-01 : (c4 ? 9.82793723247329054082e-01 : 1.57079632679489655800e+00)));
    const double lo = c1 ? 0.0 : (c2 ? 2.26987774529616870924e-17 : (c3 ? 3.06161699786838301793e-17 : (c4 ? 1.39033110312309984516e-17 : 6.12323399573676603587e-17)));
    const double z = x * x;
    const double w = z * z;
    const double s1 = z * (3.33333333333329318027e-01 + w * (1.42857142725034663711e-01 + w * (9.09088713343650656196e-02 + w * (6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
    const double s2 = w * (-1.99999999998764832476e-01 + w * (-1.11111104054623557880e-01 + w * (-7.69187620504482999495e-02 + w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))));
    const double p = x * (s1 + s2);
    const double at = hi - ((p - lo) - x);
    return Z < 0 ? 3.14159265358979311600e+00 - (at - 1.22464679914735317723e-16) : at;
}

// value of output pixel (x, y) of one view; dv1 is the row's view-ray component
template <int CH, int MODEL>
__device__ __forceinline__ int rectify_view_pixel(int x, double dv1, const uint8_t *__restrict__ src, int w, int h, int stride, const RectifyLens &lens,
                                                  const RectifyView &vw)
{
    const double dv0 = (x + 0.5 - vw.ncx) / vw.nfx;
    const double X = vw.R[0] * dv0 + vw.R[1] * dv1 + vw.R[2] * 1.0;
    const double Y = vw.R[3] * dv0 + vw.R[4] * dv1 + vw.R[5] * 1.0;
    const double Z = vw.R[6] * dv0 + vw.R[7] * dv1 + vw.R[8] * 1.0;
    double u, v;
    if (MODEL == RECTIFY_LENS_BROWN) {
        if (Z <= 0) return lens.fill;  // behind the source camera: the polynomial has nothing to say
        rectify_brown(X / Z, Y / Z, lens.fx, lens.fy, lens.cx, lens.cy, lens.k[0], lens.k[1], lens.k[2], lens.k[3], lens.k[4], u, v);
    } else {
        const double rr = X * X + Y * Y;
        const double r = sqrt(rr);
        const double th = rectify_atan2_pos(r, Z);
        if (th > lens.theta_max) return lens.fill;
        const double t2 = th * th;
        const double td = th * (1 + t2 * (lens.k[0] + t2 * (lens.k[1] + t2 * (lens.k[2] + t2 * lens.k[3]))));
        const double s = r == 0 ? 0.0 : td / r;
        u = lens.fx * (s * X) + lens.cx;
        v = lens.fy * (s * Y) + lens.cy;
    }
    return rectify_sample<CH>(u, v, src, w, h, stride, lens.fill);
}

// z0: the first view * n_frames + frame of this launch of the chain
template <int CH, int MODEL>
__global__ void __launch_bounds__(256) k_rectify_views(const uint8_t *__restrict__ src, int n_frames, int w, int h, int stride, size_t frame_pitch,
                                                       uint8_t *__restrict__ dst, int w_out, int h_out, int stride_out, size_t frame_pitch_out, int z0,
                                                       RectifyLens lens, RectifyViewTable views)
{
    const int z = z0 + (int)blockIdx.z;
    const int vi = z / n_frames, fr = z - vi * n_frames;  // vi < n_views <= RECTIFY_MAX_VIEWS: the host sizes the chain
    const int tx0 = blockIdx.x * RECTIFY_TW;
    const int ty0 = __builtin_amdgcn_readfirstlane((int)((blockIdx.y * 4 + threadIdx.y) * RECTIFY_TH));
    if (ty0 >= h_out) return;
    const int lane = threadIdx.x;
    const int x = tx0 + RECTIFY_PX * (lane & 7), y = ty0 + (lane >> 3);
    if (x >= w_out || y >= h_out) return;
    const RectifyView &vw = views.v[vi];
    const uint8_t *s = src + (size_t)fr * frame_pitch;
    const double dv1 = (y + 0.5 - vw.ncy) / vw.nfy;
    unsigned int val[RECTIFY_PX];
#pragma unroll
    for (int j = 0; j < RECTIFY_PX; j++) val[j] = x + j < w_out ? (unsigned int)rectify_view_pixel<CH, MODEL>(x + j, dv1, s, w, h, stride, lens, vw) : 0u;
    rectify_store(dst + (size_t)z * frame_pitch_out + (size_t)y * (size_t)stride_out + (size_t)x, val, x, w_out);
}
