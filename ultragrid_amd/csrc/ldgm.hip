// ldgm.hip -- LDGM forward error correction on the device: what ldgm/src/ldgm-session-cpu.cpp computes for UltraGrid's `-f ldgm`
// (rtp/ldgm.cpp), behind the C ABI ug_hip_ldgm_* (include/ug_mi355x.h) and the ldgm_gpu plugin (module/ldgm_gpu_mi355x.cpp).
//
// The code.  `pcm` is m rows of w_f ints, padded with -1: row r lists its data packets (< k), then parity k + r and k + r - 1.  A buffer is
// k data packets of ps bytes followed by m parity packets.  With s_r = XOR of the data packets of row r, parity p_r = s_0 ^ ... ^ s_r: an
// inclusive prefix XOR down the rows (the staircase; LDGM_session_cpu::encode).  Decoding recovers a packet from a row in which it is the only
// unknown member, as the XOR of the row's other members (LDGM_session_cpu::iterate).
//
// Byte j of every output depends on byte j of its inputs only, so work splits by byte columns with no ordering between workgroups.
//   Encode: two launches over (row band x column).  ldgm_rows_kernel writes s_r for the rows of its band into the parity region and the
//   band's XOR total into a scratch; ldgm_scan_kernel XORs the totals of the bands above its own (an exclusive scan, <= m / 16 loads per
//   lane, all independent) and then walks its band, turning s_r into p_r in place.
//   Decode: which packets can be recovered depends on the loss pattern and pcm only, never on the data.  The host peels to the fixpoint in
//   O(edges) (plan() below), keeps only the recoveries that missing DATA packets need, and groups them into levels: a recovery of level L
//   reads packets that were received or recovered below L.  The device then only XORs: one launch per level (no host round trip between
//   them), each lane a column of every recovery of the level.  A call in which no data packet is missing does no device work at all.
// Columns are 16, 8 or 4 bytes wide -- the widest that divides ps and the buffer's alignment (ps is only guaranteed a multiple of 4).
#include "ug_common.h"

#include <algorithm>
#include <new>
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace {

constexpr int kMaxK = 8191;          // ldgm.cpp MAX_K
constexpr int kMaxM = 65535;         // LDGM_session::param_m is an unsigned short
constexpr int kMaxWf = 128;          // ldgm-session.cpp MAX_W
constexpr int kMaxPs = 65535;        // LDGM_session::packet_size is an unsigned short
constexpr int kBandRows = 16;        // rows per band of the encoder
constexpr int kBlock = 256;

template <class V> struct Vec;
template <> struct Vec<uint32_t> {
        static __device__ __forceinline__ uint32_t zero() { return 0u; }
        static __device__ __forceinline__ uint32_t x(uint32_t a, uint32_t b) { return a ^ b; }
};
template <> struct Vec<uint2> {
        static __device__ __forceinline__ uint2 zero() { return make_uint2(0u, 0u); }
        static __device__ __forceinline__ uint2 x(uint2 a, uint2 b) { return make_uint2(a.x ^ b.x, a.y ^ b.y); }
};
template <> struct Vec<uint4> {
        static __device__ __forceinline__ uint4 zero() { return make_uint4(0u, 0u, 0u, 0u); }
        static __device__ __forceinline__ uint4 x(uint4 a, uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }
};

template <class V> __device__ __forceinline__ V ld(const uint8_t *p) { return *(const V *) p; }
template <class V> __device__ __forceinline__ void st(uint8_t *p, V v) { *(V *) p = v; }

// grid (column blocks, bands).  s_r of every row of the band -> parity row r; the band's XOR -> tot[band][column].
template <class V>
__global__ __launch_bounds__(kBlock) void ldgm_rows_kernel(uint8_t *buf, V *tot, const int *__restrict__ pcm, int k, int m, int wf, int ps, int ncols)
{
        const int c = blockIdx.x * blockDim.x + threadIdx.x;
        if (c >= ncols) return;
        const int b = blockIdx.y;
        const int r1 = min(m, (b + 1) * kBandRows);
        const size_t col = (size_t) c * sizeof(V);
        uint8_t *const parity = buf + (size_t) k * ps;
        V t = Vec<V>::zero();
        for (int r = b * kBandRows; r < r1; ++r) {
                const int *row = pcm + (size_t) r * wf; // uniform across the workgroup: scalar loads
                V s = Vec<V>::zero();
                for (int j = 0; j < wf; ++j) {
                        const int idx = row[j];
                        if ((unsigned) idx < (unsigned) k) s = Vec<V>::x(s, ld<V>(buf + (size_t) idx * ps + col));
                }
                st<V>(parity + (size_t) r * ps + col, s);
                t = Vec<V>::x(t, s);
        }
        tot[(size_t) b * ncols + c] = t;
}

// grid (column blocks, bands).  p_r = (XOR of the totals of the bands above) ^ s_(band start) ^ ... ^ s_r, in place.
template <class V>
__global__ __launch_bounds__(kBlock) void ldgm_scan_kernel(uint8_t *buf, const V *__restrict__ tot, int k, int m, int ps, int ncols)
{
        const int c = blockIdx.x * blockDim.x + threadIdx.x;
        if (c >= ncols) return;
        const int b = blockIdx.y;
        const int r1 = min(m, (b + 1) * kBandRows);
        const size_t col = (size_t) c * sizeof(V);
        uint8_t *const parity = buf + (size_t) k * ps;
        V p = Vec<V>::zero();
        for (int bb = 0; bb < b; ++bb) p = Vec<V>::x(p, tot[(size_t) bb * ncols + c]);
        for (int r = b * kBandRows; r < r1; ++r) {
                uint8_t *q = parity + (size_t) r * ps + col;
                p = Vec<V>::x(p, ld<V>(q));
                st<V>(q, p);
        }
}

// grid (recoveries of one level, column blocks).  e = (row, target): target = XOR of the row's other members (a member listed twice
// counts twice, as the reference's xor loop does; entries equal to the target are skipped, as there).
template <class V>
__global__ __launch_bounds__(kBlock) void ldgm_peel_kernel(uint8_t *buf, const int2 *__restrict__ entries, const int *__restrict__ pcm, int wf, int ps, int ncols)
{
        const int c = blockIdx.y * blockDim.x + threadIdx.x;
        if (c >= ncols) return;
        const int2 e = entries[blockIdx.x];
        const int *row = pcm + (size_t) e.x * wf;
        const size_t col = (size_t) c * sizeof(V);
        V acc = Vec<V>::zero();
        for (int j = 0; j < wf; ++j) {
                const int idx = row[j];
                if (idx >= 0 && idx != e.y) acc = Vec<V>::x(acc, ld<V>(buf + (size_t) idx * ps + col));
        }
        st<V>(buf + (size_t) e.y * ps + col, acc);
}

// grid (packets, column blocks): packet list[i] -> dst slot i (the host form's one download of the recovered data packets)
template <class V>
__global__ __launch_bounds__(kBlock) void ldgm_gather_kernel(uint8_t *dst, const uint8_t *__restrict__ buf, const int *__restrict__ list, int ps, int ncols)
{
        const int c = blockIdx.y * blockDim.x + threadIdx.x;
        if (c >= ncols) return;
        const size_t col = (size_t) c * sizeof(V);
        st<V>(dst + (size_t) blockIdx.x * ps + col, ld<V>(buf + (size_t) list[blockIdx.x] * ps + col));
}

struct DeviceGuard { // the session's device for the call, the caller's back afterwards
        int prev = -1;
        hipError_t err = hipSuccess;
        explicit DeviceGuard(int dev)
        {
                err = hipGetDevice(&prev);
                if (err == hipSuccess && prev != dev) err = hipSetDevice(dev);
        }
        ~DeviceGuard()
        {
                if (prev >= 0) (void) hipSetDevice(prev);
        }
};

template <class T> void grow_device(T *&p, size_t &cap, size_t bytes, hipError_t &err)
{
        if (cap >= bytes) return;
        if (p) (void) hipFree(p);
        p = nullptr;
        cap = 0;
        err = hipMalloc((void **) &p, bytes);
        if (err == hipSuccess) cap = bytes;
}
template <class T> void grow_host(T *&p, size_t &cap, size_t bytes, hipError_t &err)
{
        if (cap >= bytes) return;
        if (p) (void) hipHostFree(p);
        p = nullptr;
        cap = 0;
        err = hipHostMalloc((void **) &p, bytes, hipHostMallocDefault);
        if (err == hipSuccess) cap = bytes;
}

int vec_bytes(int ps, const void *buf)
{
        const uintptr_t a = (uintptr_t) buf;
        if (ps % 16 == 0 && a % 16 == 0) return 16;
        if (ps % 8 == 0 && a % 8 == 0) return 8;
        return 4;
}

} // namespace

struct ug_hip_ldgm {
        int device, k, m, wf;
        std::vector<int> pcm;                    // host copy, m x wf
        std::vector<int> row_n;                  // members (>= 0) per row
        std::vector<int> col_start, col_rows;    // rows containing packet i (with multiplicity): col_rows[col_start[i] .. col_start[i+1])
        int *pcm_dev = nullptr;
        uint8_t *tot_dev = nullptr;              // encode: band totals
        size_t tot_cap = 0;
        uint8_t *buf_dev = nullptr;              // host forms: the (k + m) x ps buffer on the device
        size_t buf_cap = 0;
        uint8_t *gather_dev = nullptr;           // decode_host: recovered data packets, back to back
        size_t gather_cap = 0;
        uint8_t *gather_host = nullptr;          // pinned
        size_t gather_host_cap = 0;
        int *sched_dev = nullptr;                // decode: (row, target) pairs, then the gather list
        size_t sched_cap = 0;
        int *sched_host = nullptr;               // pinned staging of the same
        size_t sched_host_cap = 0;
        hipEvent_t sched_copied = nullptr;       // the staging may be rewritten once this has completed
        bool sched_pending = false;
        // the plan of the last decode
        std::vector<int> cnt, entries, level_start, keep, data_rec;
        std::vector<uint8_t> known, needed;
        // diagnostics of the last call
        int launches = 0, copies = 0, levels = 0;
};

namespace {

int refuse(const char *msg)
{
        ug::set_last_error_msg(msg);
        return UG_HIP_EINVAL;
}

int check_ps(const char *who, int ps)
{
        if (ps <= 0 || ps % 4 != 0 || ps > kMaxPs) {
                char msg[160];
                snprintf(msg, sizeof msg, "%s: packet size %d is not a positive multiple of 4 up to %d", who, ps, kMaxPs);
                return refuse(msg);
        }
        return UG_HIP_SUCCESS;
}

// Peeling to the fixpoint, by levels, O(edges): a row whose members are all known but one recovers that one.  received[i] != 0: packet i
// arrived.  Fills s->entries (row, target pairs in level order, only the recoveries that missing data packets need), s->level_start
// (offsets into entries / 2, one more than the levels), s->data_rec (recovered data packets, ascending) and `recovered` / all-known.
void plan(ug_hip_ldgm *s, const uint8_t *received, uint8_t *recovered, int *all_data_known)
{
        const int n = s->k + s->m, wf = s->wf;
        s->known.assign(received, received + n);
        for (auto &v : s->known) v = v != 0;
        s->cnt.assign(s->m, 0);
        for (int r = 0; r < s->m; ++r)
                for (int j = 0; j < wf; ++j) {
                        const int idx = s->pcm[(size_t) r * wf + j];
                        if (idx >= 0 && !s->known[idx]) s->cnt[r]++;
                }
        std::vector<int> frontier, next, order, order_level; // order: (row, target) of every recovery, order_level: its level
        for (int r = 0; r < s->m; ++r)
                if (s->cnt[r] == 1 && s->row_n[r] >= 2) frontier.push_back(r);
        for (int level = 0; !frontier.empty(); ++level) {
                next.clear();
                for (int r : frontier) {
                        if (s->cnt[r] != 1) continue; // its one unknown was recovered by another row of this level
                        int t = -1;
                        for (int j = 0; j < wf && t < 0; ++j) {
                                const int idx = s->pcm[(size_t) r * wf + j];
                                if (idx >= 0 && !s->known[idx]) t = idx;
                        }
                        order.push_back(r);
                        order.push_back(t);
                        order_level.push_back(level);
                        s->known[t] = 1;
                        for (int q = s->col_start[t]; q < s->col_start[t + 1]; ++q) {
                                const int row = s->col_rows[q];
                                if (--s->cnt[row] == 1 && s->row_n[row] >= 2) next.push_back(row);
                        }
                }
                frontier.swap(next);
        }
        int all = 1;
        for (int i = 0; i < s->k; ++i) all &= s->known[i];
        if (all_data_known) *all_data_known = all;
        // prune backwards: a recovery is kept if a missing data packet needs it
        s->needed.assign(n, 0);
        for (int i = 0; i < s->k; ++i) s->needed[i] = !received[i];
        const int nrec = (int) order_level.size();
        s->keep.assign(nrec, 0);
        for (int e = nrec - 1; e >= 0; --e) {
                const int r = order[2 * e], t = order[2 * e + 1];
                if (!s->needed[t]) continue;
                s->keep[e] = 1;
                for (int j = 0; j < wf; ++j) {
                        const int idx = s->pcm[(size_t) r * wf + j];
                        if (idx >= 0 && idx != t && !received[idx]) s->needed[idx] = 1;
                }
        }
        s->entries.clear();
        s->level_start.assign(1, 0);
        s->data_rec.clear();
        if (recovered) memset(recovered, 0, n);
        int last_level = -1;
        for (int e = 0; e < nrec; ++e) {
                if (!s->keep[e]) continue;
                if (order_level[e] != last_level && last_level >= 0) s->level_start.push_back((int) s->entries.size() / 2);
                last_level = order_level[e];
                s->entries.push_back(order[2 * e]);
                s->entries.push_back(order[2 * e + 1]);
                if (recovered) recovered[order[2 * e + 1]] = 1;
                if (order[2 * e + 1] < s->k) s->data_rec.push_back(order[2 * e + 1]);
        }
        if (!s->entries.empty()) s->level_start.push_back((int) s->entries.size() / 2);
        std::sort(s->data_rec.begin(), s->data_rec.end());
        s->levels = (int) s->level_start.size() - 1;
}

template <class V>
int launch_encode(ug_hip_ldgm *s, uint8_t *buf, int ps, hipStream_t st)
{
        const int ncols = ps / (int) sizeof(V);
        const int bands = (s->m + kBandRows - 1) / kBandRows;
        hipError_t err = hipSuccess;
        grow_device(s->tot_dev, s->tot_cap, (size_t) bands * ps, err);
        UG_HIP_TRY(err);
        const int threads = std::min(kBlock, (ncols + 63) / 64 * 64);
        const dim3 grid((ncols + threads - 1) / threads, bands);
        ldgm_rows_kernel<V><<<grid, threads, 0, st>>>(buf, (V *) s->tot_dev, s->pcm_dev, s->k, s->m, s->wf, ps, ncols);
        UG_HIP_LAUNCH_CHECK();
        ldgm_scan_kernel<V><<<grid, threads, 0, st>>>(buf, (const V *) s->tot_dev, s->k, s->m, ps, ncols);
        UG_HIP_LAUNCH_CHECK();
        s->launches += 2;
        return UG_HIP_SUCCESS;
}

int encode_dev(ug_hip_ldgm *s, uint8_t *buf, int ps, hipStream_t st)
{
        switch (vec_bytes(ps, buf)) {
        case 16: return launch_encode<uint4>(s, buf, ps, st);
        case 8: return launch_encode<uint2>(s, buf, ps, st);
        default: return launch_encode<uint32_t>(s, buf, ps, st);
        }
}

template <class V>
int launch_peel(ug_hip_ldgm *s, uint8_t *buf, int ps, hipStream_t st)
{
        const int ncols = ps / (int) sizeof(V);
        const int threads = std::min(kBlock, (ncols + 63) / 64 * 64);
        const int cblocks = (ncols + threads - 1) / threads;
        const int2 *ent = (const int2 *) s->sched_dev;
        for (int l = 0; l < s->levels; ++l) {
                const int a = s->level_start[l], b = s->level_start[l + 1];
                ldgm_peel_kernel<V><<<dim3(b - a, cblocks), threads, 0, st>>>(buf, ent + a, s->pcm_dev, s->wf, ps, ncols);
                UG_HIP_LAUNCH_CHECK();
                s->launches++;
        }
        return UG_HIP_SUCCESS;
}

template <class V>
int launch_gather(ug_hip_ldgm *s, const uint8_t *buf, int ps, hipStream_t st)
{
        const int ncols = ps / (int) sizeof(V);
        const int threads = std::min(kBlock, (ncols + 63) / 64 * 64);
        const int cblocks = (ncols + threads - 1) / threads;
        const int *list = s->sched_dev + s->entries.size();
        if (s->data_rec.empty()) return UG_HIP_SUCCESS;
        ldgm_gather_kernel<V><<<dim3((unsigned) s->data_rec.size(), cblocks), threads, 0, st>>>(s->gather_dev, buf, list, ps, ncols);
        UG_HIP_LAUNCH_CHECK();
        s->launches++;
        return UG_HIP_SUCCESS;
}

// schedule (and, with_list, the gather list) -> device; the recoveries of every level
int decode_dev(ug_hip_ldgm *s, uint8_t *buf, int ps, bool with_list, hipStream_t st)
{
        const size_t words = s->entries.size() + (with_list ? s->data_rec.size() : 0);
        hipError_t err = hipSuccess;
        if (s->sched_pending) { // the previous call's upload may still read the staging buffer
                UG_HIP_TRY(hipEventSynchronize(s->sched_copied));
                s->sched_pending = false;
        }
        grow_host(s->sched_host, s->sched_host_cap, words * sizeof(int), err);
        UG_HIP_TRY(err);
        grow_device(s->sched_dev, s->sched_cap, words * sizeof(int), err);
        UG_HIP_TRY(err);
        memcpy(s->sched_host, s->entries.data(), s->entries.size() * sizeof(int));
        if (with_list) memcpy(s->sched_host + s->entries.size(), s->data_rec.data(), s->data_rec.size() * sizeof(int));
        UG_HIP_TRY(hipMemcpyAsync(s->sched_dev, s->sched_host, words * sizeof(int), hipMemcpyHostToDevice, st));
        UG_HIP_TRY(hipEventRecord(s->sched_copied, st));
        s->sched_pending = true;
        s->copies++;
        switch (vec_bytes(ps, buf)) {
        case 16: return launch_peel<uint4>(s, buf, ps, st);
        case 8: return launch_peel<uint2>(s, buf, ps, st);
        default: return launch_peel<uint32_t>(s, buf, ps, st);
        }
}

int check_call(const char *who, ug_hip_ldgm *s, const void *buf, int ps)
{
        if (int rc = check_ps(who, ps)) return rc;
        if (!s || !buf) {
                char msg[128];
                snprintf(msg, sizeof msg, "%s: NULL session or buffer", who);
                return refuse(msg);
        }
        s->launches = s->copies = s->levels = 0;
        return UG_HIP_SUCCESS;
}

} // namespace

extern "C" {

int ug_hip_ldgm_create(int device, int k, int m, const int *pcm, int w_f, ug_hip_ldgm **out)
{
        if (!out) return refuse("ug_hip_ldgm_create: NULL out");
        *out = nullptr;
        if (device < 0) return refuse("ug_hip_ldgm_create: negative device");
        if (k < 1 || k > kMaxK || m < 1 || m > kMaxM) return refuse("ug_hip_ldgm_create: k must lie in 1..8191 and m in 1..65535");
        if (w_f < 2 || w_f > kMaxWf) return refuse("ug_hip_ldgm_create: w_f must lie in 2..128");
        if (!pcm) return refuse("ug_hip_ldgm_create: NULL pcm");
        const int n = k + m;
        for (size_t i = 0; i < (size_t) m * w_f; ++i)
                if (pcm[i] < -1 || pcm[i] >= n) return refuse("ug_hip_ldgm_create: pcm entry outside [-1, k + m)");
        ug_hip_ldgm *s = new (std::nothrow) ug_hip_ldgm();
        if (!s) return refuse("ug_hip_ldgm_create: out of memory");
        s->device = device;
        s->k = k;
        s->m = m;
        s->wf = w_f;
        s->pcm.assign(pcm, pcm + (size_t) m * w_f);
        s->row_n.assign(m, 0);
        s->col_start.assign(n + 1, 0);
        for (int r = 0; r < m; ++r)
                for (int j = 0; j < w_f; ++j) {
                        const int idx = pcm[(size_t) r * w_f + j];
                        if (idx >= 0) {
                                s->row_n[r]++;
                                s->col_start[idx + 1]++;
                        }
                }
        for (int i = 0; i < n; ++i) s->col_start[i + 1] += s->col_start[i];
        s->col_rows.resize(s->col_start[n]);
        std::vector<int> fill(s->col_start.begin(), s->col_start.end() - 1);
        for (int r = 0; r < m; ++r)
                for (int j = 0; j < w_f; ++j) {
                        const int idx = pcm[(size_t) r * w_f + j];
                        if (idx >= 0) s->col_rows[fill[idx]++] = r;
                }
        DeviceGuard g(device);
        hipError_t err = g.err;
        if (err == hipSuccess) err = hipMalloc((void **) &s->pcm_dev, s->pcm.size() * sizeof(int));
        if (err == hipSuccess) err = hipMemcpy(s->pcm_dev, s->pcm.data(), s->pcm.size() * sizeof(int), hipMemcpyHostToDevice);
        if (err == hipSuccess) err = hipEventCreateWithFlags(&s->sched_copied, hipEventDisableTiming);
        if (err != hipSuccess) {
                ug::set_last_error(err, "ug_hip_ldgm_create");
                ug_hip_ldgm_destroy(s);
                return UG_HIP_ERUNTIME;
        }
        *out = s;
        return UG_HIP_SUCCESS;
}

void ug_hip_ldgm_destroy(ug_hip_ldgm *s)
{
        if (!s) return;
        DeviceGuard g(s->device);
        if (s->sched_copied) {
                (void) hipEventSynchronize(s->sched_copied);
                (void) hipEventDestroy(s->sched_copied);
        }
        for (void *p : {(void *) s->pcm_dev, (void *) s->tot_dev, (void *) s->buf_dev, (void *) s->gather_dev, (void *) s->sched_dev})
                if (p) (void) hipFree(p);
        for (void *p : {(void *) s->gather_host, (void *) s->sched_host})
                if (p) (void) hipHostFree(p);
        delete s;
}

int ug_hip_ldgm_encode(ug_hip_ldgm *s, void *buf_dev, int ps, ug_hip_stream_t stream)
{
        if (int rc = check_call("ug_hip_ldgm_encode", s, buf_dev, ps)) return rc;
        DeviceGuard g(s->device);
        UG_HIP_TRY(g.err);
        return encode_dev(s, (uint8_t *) buf_dev, ps, (hipStream_t) stream);
}

int ug_hip_ldgm_decode(ug_hip_ldgm *s, void *buf_dev, int ps, const uint8_t *received, uint8_t *recovered, int *all_data_known,
                       ug_hip_stream_t stream)
{
        if (int rc = check_call("ug_hip_ldgm_decode", s, buf_dev, ps)) return rc;
        if (!received) return refuse("ug_hip_ldgm_decode: NULL received mask");
        plan(s, received, recovered, all_data_known);
        if (s->entries.empty()) return UG_HIP_SUCCESS; // nothing missing, or nothing recoverable: no device work
        DeviceGuard g(s->device);
        UG_HIP_TRY(g.err);
        return decode_dev(s, (uint8_t *) buf_dev, ps, false, (hipStream_t) stream);
}

int ug_hip_ldgm_encode_host(ug_hip_ldgm *s, void *buf_host, int ps, ug_hip_stream_t stream)
{
        if (int rc = check_call("ug_hip_ldgm_encode_host", s, buf_host, ps)) return rc;
        DeviceGuard g(s->device);
        UG_HIP_TRY(g.err);
        hipStream_t st = (hipStream_t) stream;
        hipError_t err = hipSuccess;
        const size_t data = (size_t) s->k * ps, par = (size_t) s->m * ps;
        grow_device(s->buf_dev, s->buf_cap, data + par, err);
        UG_HIP_TRY(err);
        UG_HIP_TRY(hipMemcpyAsync(s->buf_dev, buf_host, data, hipMemcpyHostToDevice, st));
        s->copies++;
        if (int rc = encode_dev(s, s->buf_dev, ps, st)) return rc;
        UG_HIP_TRY(hipMemcpyAsync((uint8_t *) buf_host + data, s->buf_dev + data, par, hipMemcpyDeviceToHost, st));
        s->copies++;
        UG_HIP_TRY(hipStreamSynchronize(st));
        return UG_HIP_SUCCESS;
}

int ug_hip_ldgm_decode_host(ug_hip_ldgm *s, void *buf_host, int ps, const uint8_t *received, uint8_t *recovered, int *all_data_known,
                            ug_hip_stream_t stream)
{
        if (int rc = check_call("ug_hip_ldgm_decode_host", s, buf_host, ps)) return rc;
        if (!received) return refuse("ug_hip_ldgm_decode_host: NULL received mask");
        plan(s, received, recovered, all_data_known);
        if (s->entries.empty()) return UG_HIP_SUCCESS;
        DeviceGuard g(s->device);
        UG_HIP_TRY(g.err);
        hipStream_t st = (hipStream_t) stream;
        hipError_t err = hipSuccess;
        const size_t all = (size_t) (s->k + s->m) * ps, got = s->data_rec.size() * (size_t) ps;
        grow_device(s->buf_dev, s->buf_cap, all, err);
        UG_HIP_TRY(err);
        grow_device(s->gather_dev, s->gather_cap, got, err);
        UG_HIP_TRY(err);
        grow_host(s->gather_host, s->gather_host_cap, got, err);
        UG_HIP_TRY(err);
        UG_HIP_TRY(hipMemcpyAsync(s->buf_dev, buf_host, all, hipMemcpyHostToDevice, st));
        s->copies++;
        if (int rc = decode_dev(s, s->buf_dev, ps, true, st)) return rc;
        int rc;
        switch (vec_bytes(ps, s->buf_dev)) {
        case 16: rc = launch_gather<uint4>(s, s->buf_dev, ps, st); break;
        case 8: rc = launch_gather<uint2>(s, s->buf_dev, ps, st); break;
        default: rc = launch_gather<uint32_t>(s, s->buf_dev, ps, st); break;
        }
        if (rc) return rc;
        UG_HIP_TRY(hipMemcpyAsync(s->gather_host, s->gather_dev, got, hipMemcpyDeviceToHost, st));
        s->copies++;
        UG_HIP_TRY(hipStreamSynchronize(st));
        for (size_t i = 0; i < s->data_rec.size(); ++i)
                memcpy((uint8_t *) buf_host + (size_t) s->data_rec[i] * ps, s->gather_host + i * ps, ps);
        return UG_HIP_SUCCESS;
}

int ug_hip_ldgm_stats(const ug_hip_ldgm *s, int *launches, int *copies, int *levels)
{
        if (!s) return refuse("ug_hip_ldgm_stats: NULL session");
        if (launches) *launches = s->launches;
        if (copies) *copies = s->copies;
        if (levels) *levels = s->levels;
        return UG_HIP_SUCCESS;
}

} // extern "C"
