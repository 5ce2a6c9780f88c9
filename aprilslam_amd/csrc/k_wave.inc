// Cross-lane primitives of the kernels: DPP moves, lane exchanges, readlane, the wave scan, reduction and prefix sum, the maximum,
// minimum and owner of a group of 8 lanes, butterfly sums.
// They need neither LDS nor an address register: ds_bpermute does the same in ~100 cycles of latency per exchange, and a
// sorting network or a reduction is a chain of such exchanges.
// lane_xor<J>: value of lane (l ^ J) for a compile-time J, 32- or 64-bit.
//   J = 1, 2   DPP quad_perm                         (one v_mov_b32_dpp per dword)
//   J = 4      DPP row_shl:4 / row_shr:4 by bank     (two)
//   J = 8      DPP row_ror:8                         (one)
//   J = 16, 32 v_permlane16_swap / v_permlane32_swap (gfx950: swaps odd rows / the upper half of one operand with even
//              rows / the lower half of the other; with both operands the same value the partner is in one of the two)
// After a butterfly sum (butterfly_sum) every lane holds the same bits -- a + b is commutative, and the order of the
// additions is fixed -- so serial work that follows it can run redundantly in all lanes on identical inputs, without a
// broadcast, and the result does not depend on the run.

// DPP control words: quad_perm [a,b,c,d] = a | b << 2 | c << 4 | d << 6 (lane q of a quad takes the value of lane [q])
#define QUAD_XOR1 0xB1 /* quad_perm [1,0,3,2]: value of lane l ^ 1 */
#define QUAD_XOR2 0x4E /* quad_perm [2,3,0,1]: value of lane l ^ 2 */
#define QUAD_ROT1 0x39 /* quad_perm [1,2,3,0]: value of lane l + 1 */
#define QUAD_ROT2 0x4E /* quad_perm [2,3,0,1]: value of lane l + 2 */
#define QUAD_ROT3 0x93 /* quad_perm [3,0,1,2]: value of lane l + 3 */
#define ROW_HALF_MIRROR 0x141 /* row_half_mirror: lane i of each 8 takes the value of lane 7 - i, in the group's other quad */

// One DPP move of a 32- or 64-bit value (a 64-bit value moves as two dwords): lanes whose source lies outside the row, or
// whose row or bank is masked, receive `old`.
template <int CTRL, int ROWMASK = 0xf, int BANKMASK = 0xf, typename T>
__device__ __forceinline__ T dpp_mov(T old, T v)
{
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "32- or 64-bit values");
    if constexpr (sizeof(T) == 4) {
        return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL, ROWMASK, BANKMASK, false));
    } else {
        const unsigned long long ou = __builtin_bit_cast(unsigned long long, old), vu = __builtin_bit_cast(unsigned long long, v);
        const unsigned int lo = (unsigned int)__builtin_amdgcn_update_dpp((int)(unsigned int)ou, (int)(unsigned int)vu, CTRL, ROWMASK, BANKMASK, false);
        const unsigned int hi = (unsigned int)__builtin_amdgcn_update_dpp((int)(unsigned int)(ou >> 32), (int)(unsigned int)(vu >> 32), CTRL, ROWMASK, BANKMASK, false);
        return __builtin_bit_cast(T, ((unsigned long long)hi << 32) | lo);
    }
}

// value of lane K of the quad (quad_perm [K,K,K,K])
template <int K, typename T>
__device__ __forceinline__ T quad_bcast(T v)
{
    return dpp_mov<K * 0x55>(T(0), v);
}

// value of lane l (wave-uniform) of a 32- or 64-bit value
template <typename T>
__device__ __forceinline__ T readlane(T v, int l)
{
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "32- or 64-bit values");
    if constexpr (sizeof(T) == 4) {
        return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
    } else {
        const unsigned long long vu = __builtin_bit_cast(unsigned long long, v);
        const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)vu, l), hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(vu >> 32), l);
        return __builtin_bit_cast(T, ((unsigned long long)hi << 32) | lo);
    }
}

template <int J>
__device__ __forceinline__ unsigned int lane_xor32(unsigned int v)
{
    static_assert(J == 1 || J == 2 || J == 4 || J == 8 || J == 16 || J == 32, "power of two below 64");
    if constexpr (J == 1) return (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);  // quad_perm [1,0,3,2]
    else if constexpr (J == 2) return (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);  // quad_perm [2,3,0,1]
    else if constexpr (J == 4) {
        const int t = __builtin_amdgcn_update_dpp((int)v, (int)v, 0x104, 0xf, 0x5, false);  // row_shl:4 into banks 0 and 2 (lane bit 2 clear): from l + 4
        return (unsigned int)__builtin_amdgcn_update_dpp(t, (int)v, 0x114, 0xf, 0xA, false);  // row_shr:4 into banks 1 and 3: from l - 4
    } else if constexpr (J == 8) return (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);  // row_ror:8
    else if constexpr (J == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);  // r[0]: rows 0,0,2,2 of v; r[1]: rows 1,1,3,3
        return (__lane_id() & 16u) ? r[0] : r[1];
    } else {
        const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);  // r[0]: lower half twice; r[1]: upper half twice
        return (__lane_id() & 32u) ? r[0] : r[1];
    }
}

template <int J>
__device__ __forceinline__ unsigned long long lane_xor(unsigned long long v)
{
    return ((unsigned long long)lane_xor32<J>((unsigned int)(v >> 32)) << 32) | lane_xor32<J>((unsigned int)v);
}

// Inclusive scan of op over the 64 lanes (lane l: v_0 op ... op v_l, left to right); all lanes must be active.  REDUCE: the
// reduction instead, lane 63's value in every lane.  (A wave_reduce wrapper around it would be one more inline level, and
// that lets the optimiser reorder the 64-bit adds of block_reduce in k_fit_quads.)
template <bool REDUCE, typename T, typename Op>
__device__ __forceinline__ T wave_scan(T v, T ident, Op op)
{
    v = op(v, dpp_mov<0x111>(ident, v));       // row_shr:1
    v = op(v, dpp_mov<0x112>(ident, v));       // row_shr:2
    v = op(v, dpp_mov<0x114>(ident, v));       // row_shr:4
    v = op(v, dpp_mov<0x118>(ident, v));       // row_shr:8   -> scans inside every row of 16 lanes
    v = op(v, dpp_mov<0x142, 0xa>(ident, v));  // row_bcast:15 into rows 1 and 3
    v = op(v, dpp_mov<0x143, 0xc>(ident, v));  // row_bcast:31 into rows 2 and 3 -> lane 63 holds the whole wave's result
    if constexpr (REDUCE) return readlane(v, 63);
    else return v;
}

// Exclusive prefix sum of an int over the 64 lanes (lane l: v_0 + ... + v_{l-1}) and, in every lane, the wave's sum in
// *total; all lanes must be active.
__device__ __forceinline__ int wave_prefix_sum(int v, int *total)
{
    const int incl = wave_scan<false>(v, 0, [](int a, int b) { return a + b; });
    *total = readlane(incl, 63);
    return incl - v;
}

// Groups of 8 lanes (k_homography: one quad per group).  Maximum resp. minimum over the group, in all 8 lanes: the other
// lanes of the quad through xor 1 and xor 2, the other quad through the half-row mirror.
__device__ __forceinline__ double grp8_max(double v)
{
    v = fmax(v, dpp_mov<QUAD_XOR1>(0.0, v));
    v = fmax(v, dpp_mov<QUAD_XOR2>(0.0, v));
    return fmax(v, dpp_mov<ROW_HALF_MIRROR>(0.0, v));
}
__device__ __forceinline__ int grp8_min(int v)
{
    v = min(v, dpp_mov<QUAD_XOR1>(0, v));
    v = min(v, dpp_mov<QUAD_XOR2>(0, v));
    return min(v, dpp_mov<ROW_HALF_MIRROR>(0, v));
}
// the lane of the group for which `mine` holds (exactly one per group), in all 8 lanes
__device__ __forceinline__ int grp8_owner(bool mine, int lane)
{
    const unsigned long long m = __ballot(mine);
    return (lane & ~7) + (__ffs((int)((m >> (lane & ~7)) & 0xFFull)) - 1);
}

// sum of a double or an int over each aligned group of LANES lanes, in every lane of the group: the exchanges with
// lane l ^ 1, l ^ 2, ..., l ^ LANES/2, added in that order
template <int LANES, typename T>
__device__ __forceinline__ T butterfly_sum(T v)
{
    static_assert(LANES == 1 || LANES == 2 || LANES == 4 || LANES == 8 || LANES == 16 || LANES == 32 || LANES == 64, "power of two up to 64");
    static_assert(__is_same(T, double) || __is_same(T, int), "double or int");
    if constexpr (LANES > 1) {
        v = butterfly_sum<LANES / 2>(v);
        if constexpr (sizeof(T) == 8) v += __builtin_bit_cast(double, lane_xor<LANES / 2>(__builtin_bit_cast(unsigned long long, v)));
        else v += (int)lane_xor32<LANES / 2>((unsigned int)v);
    }
    return v;
}
