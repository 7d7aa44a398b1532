// halo.hip -- halo exchange of the row-sharded lattice step (cbf_amd/shard.py): pack the
// owned edge rows and the guard records, unpack the neighbours' rows into the window, and the halo
// guard over every rank's records (gfx950).  Two buffer layouts: the gathered one (all-gather of
// equal slabs) and the neighbour one (one all_to_all_single of per-destination chunks).
#include "cbf_device.hpp"
#include "lattice_ego.hpp"

using namespace cbf;

namespace {

inline int nblk(long n) { return (int)((n + kBlock - 1) / kBlock); }

__device__ __forceinline__ double dkey_inv(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return __longlong_as_double((long long)u);
}

__device__ __forceinline__ unsigned long long ext_identity(int v) {
    return dkey(ext_is_min(v) ? INFINITY : -INFINITY);
}

// The kExtVals extent keys of sub-step q reduced over its kExtSlots slots (lane l of a full wave;
// every lane gets the result); the slots are left at the identity for the next accumulation.
struct ExtKeys {
    unsigned long long k[kExtVals];
};
__device__ __forceinline__ ExtKeys ext_keys_take(unsigned long long* __restrict__ keys, int q, int l) {
    ExtKeys R;
#pragma unroll
    for (int v = 0; v < kExtVals; ++v) R.k[v] = ext_identity(v);
    for (int j = l; j < kExtSlots; j += 64) {
        unsigned long long* kl = keys + (long)kExtSlotWords * (kExtSlots * q + j);
#pragma unroll
        for (int v = 0; v < kExtVals; ++v) {
            const unsigned long long x = kl[v];
            R.k[v] = ext_is_min(v) ? (x < R.k[v] ? x : R.k[v]) : (x > R.k[v] ? x : R.k[v]);
            kl[v] = ext_identity(v);
        }
    }
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int v = 0; v < kExtVals; ++v) {
            const unsigned long long x = __shfl_xor(R.k[v], o, 64);
            R.k[v] = ext_is_min(v) ? (x < R.k[v] ? x : R.k[v]) : (x > R.k[v] ? x : R.k[v]);
        }
    return R;
}

__global__ void k_ext_reset(unsigned long long* __restrict__ keys, int nsub) {
    for (int i = threadIdx.x; i < kExtSlots * nsub; i += blockDim.x) {
        unsigned long long* kl = keys + (long)kExtSlotWords * i;
#pragma unroll
        for (int v = 0; v < kExtVals; ++v) kl[v] = ext_identity(v);
    }
}

// Chunk q of a neighbour-exchange buffer: rank r sends its first G rows to r-1 and its last G rows
// to r+1 only, and its nsub guard records (8 doubles each) to every rank, which the guard needs
// from all of them.  Chunk q of the send buffer (to rank q) and of the receive buffer (from rank q)
// are [records (r8 = 8 nsub) | rows (rs2 = 2 G W doubles) if q = r +- 1]: the two layouts have the
// same sizes, so one offset formula serves both (cbf_amd/shard.py: ShardedLattice.nbr_splits).
__device__ __forceinline__ long nbr_chunk_off(int q, int rank, int ws, long r8, long rs2) {
    long o = (long)q * r8;
    if (rank > 0 && q > rank - 1) o += rs2;
    if (rank + 1 < ws && q > rank + 1) o += rs2;
    return o;
}

// Where rank q's guard record of one sub-step lives: in the gathered layout at a fixed stride from
// the record of rank 0; in the neighbour layout at 8 s into chunk q.
struct GatheredRec {
    const double* rec0;
    long stride;
    __device__ const double* operator()(int q) const { return rec0 + (long)q * stride; }
};
struct NbrRec {
    const double* recv;
    int s, ws, rank;
    long r8, rs2;
    __device__ const double* operator()(int q) const { return recv + nbr_chunk_off(q, rank, ws, r8, rs2) + 8 * s; }
};

// The halo guard of one sub-step: every agent outside rank's candidate rows is farther than the
// cull radius (in y) from every agent rank computed.  rec(q) is rank q's record: {min y, max y of
// q's computed rows, max y of q's owned rows below its top `guard` rows, min y above its bottom
// `guard` rows[, min y, max y of q's owned rows]}.  An adjacent rank is bounded by fields 2 / 3
// (its rows outside our candidate band), a non-adjacent one by FAR_MAX (lower ranks) / FAR_MIN
// (higher ranks).  The callers differ, on purpose:
//   k_halo_guard (cbf_halo_guard)  4-value records of the computed rows at a stride: far ranks by
//                                  fields 1 / 0, no identity shortcut, flag set with a plain |=;
//   k_halo_unpack, _unpack_nbr     6-value records: far ranks by their owned rows' fields 5 / 4,
//                                  a rank that recorded no computed agent (IDENT_OK: its own
//                                  record is the identity, !(ymin <= ymax)) passes, atomicOr.
template <int FAR_MAX, int FAR_MIN, bool IDENT_OK, class Rec>
__device__ __forceinline__ bool halo_guard_ok(Rec rec, int ws, int rank, double radius) {
    const double rm = radius * (1.0 + 1e-9) + 1e-12;
    const double* me = rec(rank);
    const double ymin = me[0], ymax = me[1];
    if (IDENT_OK && !(ymin <= ymax)) return true;
    bool ok = true;
    for (int q = 0; q < ws; ++q) {
        const double* o = rec(q);
        if (q < rank) {
            const double lim = (q == rank - 1) ? o[2] : o[FAR_MAX];
            if (!(ymin - lim > rm)) ok = false;
        } else if (q > rank) {
            const double lim = (q == rank + 1) ? o[3] : o[FAR_MIN];
            if (!(lim - ymax > rm)) ok = false;
        }
    }
    return ok;
}

__global__ void k_halo_guard(const double* __restrict__ E, long stride, int ws, int rank, double radius,
                             int32_t* __restrict__ flag) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (!halo_guard_ok<1, 0, false>(GatheredRec{E, stride}, ws, rank, radius)) flag[0] |= 1;
}

// ---- gathered layout: send = [first halo rows | last halo rows | nsub records of 8 doubles (6
// extents used)]; wave q of block 0 (q < nsub) writes the record of sub-step q.
__global__ void __launch_bounds__(kBlock) k_halo_pack(int W, int halo, long n_own, const double2* __restrict__ own,
                                                      unsigned long long* __restrict__ keys, int nsub,
                                                      double* __restrict__ send) {
    const long t = (long)blockIdx.x * kBlock + threadIdx.x;
    const long rs = (long)halo * W;
    double2* s2 = reinterpret_cast<double2*>(send);
    if (t < rs) s2[t] = own[t];
    else if (t < 2 * rs) s2[t] = own[n_own - 2 * rs + t];
    if (blockIdx.x == 0) {
        const int l = threadIdx.x & 63;
        for (int q = threadIdx.x >> 6; q < nsub; q += kBlock / 64) {
            const ExtKeys R = ext_keys_take(keys, q, l);
            if (l == 0) {
                double* e = send + 4 * rs + 8 * q;
#pragma unroll
                for (int v = 0; v < kExtVals; ++v) e[v] = dkey_inv(R.k[v]);
            }
        }
    }
}

// Window halo rows from the gathered slabs (rank-1's last rows below, rank+1's first rows above);
// block 0 lanes s < nsub run the guard of sub-step s on the gathered records.
__global__ void __launch_bounds__(kBlock) k_halo_unpack(int W, int halo, int rows_lo, int rows_hi, long hi_off,
                                                        const double* __restrict__ recv, long stride, int ws, int rank,
                                                        double radius, int nsub, double2* __restrict__ wpos,
                                                        int32_t* __restrict__ flag) {
    const long t = (long)blockIdx.x * kBlock + threadIdx.x;
    const long nlo = (long)rows_lo * W, nhi = (long)rows_hi * W, rs = (long)halo * W;
    if (t < nlo) {
        const double2* src = reinterpret_cast<const double2*>(recv + (long)(rank - 1) * stride) + rs + (rs - nlo);
        wpos[t] = src[t];
    } else if (t < nlo + nhi) {
        const double2* src = reinterpret_cast<const double2*>(recv + (long)(rank + 1) * stride);
        wpos[hi_off + (t - nlo)] = src[t - nlo];
    }
    if (blockIdx.x == 0 && threadIdx.x < nsub &&
        !halo_guard_ok<5, 4, true>(GatheredRec{recv + 4 * rs + 8 * threadIdx.x, stride}, ws, rank, radius))
        atomicOr(flag, 1);
}

// ---- neighbour layout (nbr_chunk_off).  Rows: thread t < n_lo copies the first G rows (to rank -
// 1), the next n_hi the last G rows (to rank + 1); block 0 writes the records into every chunk.
__global__ void __launch_bounds__(kBlock) k_halo_pack_nbr(int W, int halo, long n_own, const double2* __restrict__ own,
                                                          unsigned long long* __restrict__ keys, int nsub, int ws,
                                                          int rank, double* __restrict__ send) {
    const long t = (long)blockIdx.x * kBlock + threadIdx.x;
    const long rs = (long)halo * W, r8 = 8l * nsub;
    const long n_lo = rank > 0 ? rs : 0, n_hi = rank + 1 < ws ? rs : 0;
    if (t < n_lo) {
        reinterpret_cast<double2*>(send + nbr_chunk_off(rank - 1, rank, ws, r8, 2 * rs) + r8)[t] = own[t];
    } else if (t < n_lo + n_hi) {
        const long i = t - n_lo;
        reinterpret_cast<double2*>(send + nbr_chunk_off(rank + 1, rank, ws, r8, 2 * rs) + r8)[i] = own[n_own - rs + i];
    }
    if (blockIdx.x == 0) {
        const int l = threadIdx.x & 63;
        for (int q = threadIdx.x >> 6; q < nsub; q += kBlock / 64) {
            const ExtKeys R = ext_keys_take(keys, q, l);
            // lane d writes the record into the chunks of destinations d, d + 64, ...
            for (int d = l; d < ws; d += 64) {
                double* e = send + nbr_chunk_off(d, rank, ws, r8, 2 * rs) + 8 * q;
#pragma unroll
                for (int v = 0; v < kExtVals; ++v) e[v] = dkey_inv(R.k[v]);
            }
        }
    }
}

// Window ghost rows from the neighbours' chunks (rank-1's last rows_lo rows below, rank+1's first
// rows_hi rows above); block 0 lanes s < nsub run the guard of sub-step s.
__global__ void __launch_bounds__(kBlock) k_halo_unpack_nbr(int W, int halo, int rows_lo, int rows_hi, long hi_off,
                                                            const double* __restrict__ recv, int ws, int rank,
                                                            double radius, int nsub, double2* __restrict__ wpos,
                                                            int32_t* __restrict__ flag) {
    const long t = (long)blockIdx.x * kBlock + threadIdx.x;
    const long nlo = (long)rows_lo * W, nhi = (long)rows_hi * W, rs = (long)halo * W, r8 = 8l * nsub;
    if (t < nlo) {
        const double2* src = reinterpret_cast<const double2*>(recv + nbr_chunk_off(rank - 1, rank, ws, r8, 2 * rs) + r8);
        wpos[t] = src[rs - nlo + t];
    } else if (t < nlo + nhi) {
        const double2* src = reinterpret_cast<const double2*>(recv + nbr_chunk_off(rank + 1, rank, ws, r8, 2 * rs) + r8);
        wpos[hi_off + (t - nlo)] = src[t - nlo];
    }
    if (blockIdx.x == 0 && threadIdx.x < nsub &&
        !halo_guard_ok<5, 4, true>(NbrRec{recv, (int)threadIdx.x, ws, rank, r8, 2 * rs}, ws, rank, radius))
        atomicOr(flag, 1);
}

}  // namespace

extern "C" int cbf_halo_guard(const double* ext_all, int64_t stride, int32_t world_size, int32_t rank, double radius,
                              int32_t* flag, void* stream) {
    if (!ext_all || !flag || world_size < 1 || rank < 0 || rank >= world_size || stride < 4) return CBF_EINVAL;
    hipLaunchKernelGGL(k_halo_guard, dim3(1), dim3(64), 0, (hipStream_t)stream, ext_all, (long)stride, world_size,
                       rank, radius, flag);
    return (int)hipGetLastError();
}

extern "C" size_t cbf_halo_ext_bytes(int32_t nsub) {
    return nsub < 1 ? 0 : (size_t)nsub * kExtSlots * kExtSlotWords * sizeof(unsigned long long);
}

extern "C" int cbf_halo_ext_reset(uint64_t* ext_keys, int32_t nsub, void* stream) {
    if (!ext_keys || nsub < 1) return CBF_EINVAL;
    hipLaunchKernelGGL(k_ext_reset, dim3(1), dim3(kBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<unsigned long long*>(ext_keys), nsub);
    return (int)hipGetLastError();
}

extern "C" int cbf_halo_pack(int32_t W, int32_t halo, int64_t n_own, const double* own, uint64_t* ext_keys,
                             int32_t nsub, double* send, void* stream) {
    if (W <= 0 || halo <= 0 || n_own < 2l * halo * W || !own || !ext_keys || !send || nsub < 1) return CBF_EINVAL;
    const long n = 2l * halo * W;
    hipLaunchKernelGGL(k_halo_pack, dim3(nblk(n)), dim3(kBlock), 0, (hipStream_t)stream, W, halo, (long)n_own,
                       reinterpret_cast<const double2*>(own), reinterpret_cast<unsigned long long*>(ext_keys), nsub,
                       send);
    return (int)hipGetLastError();
}

extern "C" int cbf_halo_unpack(int32_t W, int32_t halo, int32_t rows_lo, int32_t rows_hi, int64_t hi_row_offset,
                               const double* recv, int64_t stride, int32_t world_size, int32_t rank, double radius,
                               int32_t nsub, double* wpos, int32_t* flag, void* stream) {
    if (W <= 0 || halo <= 0 || rows_lo < 0 || rows_hi < 0 || rows_lo > halo || rows_hi > halo || !recv || !wpos ||
        !flag || world_size < 1 || rank < 0 || rank >= world_size || nsub < 1 || nsub > 64 ||
        stride < 4l * halo * W + 8l * nsub || (rows_lo > 0 && rank == 0) || (rows_hi > 0 && rank == world_size - 1) ||
        hi_row_offset < 0)
        return CBF_EINVAL;
    const long n = (long)(rows_lo + rows_hi) * W;
    hipLaunchKernelGGL(k_halo_unpack, dim3(nblk(n > 0 ? n : 1)), dim3(kBlock), 0, (hipStream_t)stream, W, halo,
                       rows_lo, rows_hi, (long)hi_row_offset * W, recv, (long)stride, world_size, rank, radius, nsub,
                       reinterpret_cast<double2*>(wpos), flag);
    return (int)hipGetLastError();
}

extern "C" int64_t cbf_halo_nbr_elems(int32_t W, int32_t halo, int32_t nsub, int32_t world_size, int32_t rank) {
    if (W <= 0 || halo <= 0 || nsub < 1 || world_size < 1 || rank < 0 || rank >= world_size) return -1;
    const long r8 = 8l * nsub, rs2 = 2l * halo * W;
    return (int64_t)(world_size * r8 + (rank > 0 ? rs2 : 0) + (rank + 1 < world_size ? rs2 : 0));
}

extern "C" int cbf_halo_pack_nbr(int32_t W, int32_t halo, int64_t n_own, const double* own, uint64_t* ext_keys,
                                 int32_t nsub, int32_t world_size, int32_t rank, double* send, void* stream) {
    if (W <= 0 || halo <= 0 || n_own < 2l * halo * W || !own || !ext_keys || !send || nsub < 1 || nsub > 64 ||
        world_size < 1 || rank < 0 || rank >= world_size)
        return CBF_EINVAL;
    const long rs = (long)halo * W;
    const long n = (rank > 0 ? rs : 0) + (rank + 1 < world_size ? rs : 0);
    hipLaunchKernelGGL(k_halo_pack_nbr, dim3(nblk(n > 0 ? n : 1)), dim3(kBlock), 0, (hipStream_t)stream, W, halo,
                       (long)n_own, reinterpret_cast<const double2*>(own),
                       reinterpret_cast<unsigned long long*>(ext_keys), nsub, world_size, rank, send);
    return (int)hipGetLastError();
}

extern "C" int cbf_halo_unpack_nbr(int32_t W, int32_t halo, int32_t rows_lo, int32_t rows_hi, int64_t hi_row_offset,
                                   const double* recv, int32_t world_size, int32_t rank, double radius, int32_t nsub,
                                   double* wpos, int32_t* flag, void* stream) {
    if (W <= 0 || halo <= 0 || rows_lo < 0 || rows_hi < 0 || rows_lo > halo || rows_hi > halo || !recv || !wpos ||
        !flag || world_size < 1 || rank < 0 || rank >= world_size || nsub < 1 || nsub > 64 ||
        (rows_lo > 0 && rank == 0) || (rows_hi > 0 && rank == world_size - 1) || hi_row_offset < 0)
        return CBF_EINVAL;
    const long n = (long)(rows_lo + rows_hi) * W;
    hipLaunchKernelGGL(k_halo_unpack_nbr, dim3(nblk(n > 0 ? n : 1)), dim3(kBlock), 0, (hipStream_t)stream, W, halo,
                       rows_lo, rows_hi, (long)hi_row_offset * W, recv, world_size, rank, radius, nsub,
                       reinterpret_cast<double2*>(wpos), flag);
    return (int)hipGetLastError();
}
