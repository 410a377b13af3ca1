/**
 * @file ldgm_gpu_mi355x.cpp
 * UltraGrid's "ldgm_gpu" library (`--param ldgm-device=GPU`, src/rtp/ldgm.cpp:216-234) backed by libug_mi355x.so: an LDGM_session whose
 * encode and decode_frame run the ug_hip_ldgm_* coder (csrc/ldgm.hip) on an MI355X.  It stands where the reference's CUDA
 * LDGM_session_gpu (ldgm/src/ldgm-session-gpu.cpp, gpu.cu) stands, for the video and audio FEC of both the sender and the receiver.
 *
 *  - Device: --param mi355x-device=<n> (the first listed), else -D, else 0 -- as the MI355X receiving modules (mi355x_receiver.h).
 *  - Output buffers (alloc_buf / free_out_buf) are pinned host memory from a pool.  Frames are disposed through a callback of the frame
 *    (ldgm::encode_video_frame), on another thread than the one encoding: the pool has a mutex.
 *  - encode uploads the k x ps data bytes and downloads the m x ps parity bytes (ug_hip_ldgm_encode_host), byte for byte what
 *    LDGM_session_cpu::encode computes.  A frame whose packet size does not fit LDGM_session::packet_size (an unsigned short) is refused
 *    with a message, its parity left as encode_hdr_frame zeroed it, instead of being coded on the truncated size.
 *  - decode_frame takes the received packets by the CPU session's valid_data rule, zeroes the missing data packets as it does, and -- only
 *    when a data packet is missing -- uploads the buffer, peels on the device and downloads the recovered data packets into their places
 *    (ug_hip_ldgm_decode_host).  It recovers every packet the CPU session's 4 sweeps recover, and can recover more: it peels to the fixpoint.
 *    Parity packets are not written back (nothing reads them after decode_frame).
 */
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "debug.h"
#include "host.h"
#include "lib_common.h"
#include "rtp/ldgm.hpp"

#include "../ldgm/src/ldgm-session.h"

#include "../../include/ug_mi355x.h"
#include "mi355x_receiver.h"

#define MOD_NAME "[LDGM MI355X] "

namespace {

constexpr int kMaxPooled = 8; // free pinned buffers kept for reuse

class LDGM_session_mi355x final : public LDGM_session {
public:
        LDGM_session_mi355x()
        {
                int devs[MI355X_MAX_DEVICES];
                bool bad = false;
                mi355x_receiver_devices(devs, MI355X_MAX_DEVICES, &bad);
                if (bad) {
                        MSG(WARNING, "--param " MI355X_DEVICE_PARAM " is not a device list, using device %d\n", devs[0]);
                }
                m_device = devs[0];
        }
        ~LDGM_session_mi355x() override
        {
                ug_hip_ldgm_destroy(m_session);
                if (m_stream) {
                        ug_hip_stream_destroy(m_stream);
                }
                for (auto &b : m_free) {
                        ug_hip_free_host(b.second);
                }
        }

        void encode(char *data, char *parity) override
        {
                std::lock_guard<std::mutex> lk(m_code_mtx);
                if (!ready()) {
                        return;
                }
                // the true packet size follows from the size header encode_hdr_frame wrote (ldgm-session.cpp:254-268)
                int32_t payload = 0;
                memcpy(&payload, data, sizeof payload);
                const long long align = 4LL * param_k;
                const long long ps = (payload + 4LL + align - 1) / align * align / param_k;
                if (ps != packet_size || parity != data + (size_t) param_k * packet_size) {
                        MSG(ERROR, "frame of %d B needs %lld B packets with k=%d: LDGM packets hold at most 65535 B -- parity not computed "
                                   "(raise k)\n", (int) payload, ps, (int) param_k);
                        return;
                }
                if (ug_hip_ldgm_encode_host(m_session, data, packet_size, m_stream) != UG_HIP_SUCCESS) {
                        MSG(ERROR, "encode: %s\n", ug_hip_last_error_string());
                }
        }
        void encode_naive(char *data, char *parity) override { encode(data, parity); }

        void *alloc_buf(int size) override
        {
                if (size <= 0) {
                        return nullptr;
                }
                {
                        std::lock_guard<std::mutex> lk(m_pool_mtx);
                        auto it = m_free.lower_bound((size_t) size);
                        if (it != m_free.end()) {
                                void *p = it->second;
                                m_free.erase(it);
                                return p;
                        }
                }
                void *p = nullptr;
                if (ug_hip_malloc_host(&p, (size_t) size) != UG_HIP_SUCCESS) {
                        MSG(ERROR, "pinned buffer of %d B: %s\n", size, ug_hip_last_error_string());
                        return nullptr;
                }
                std::lock_guard<std::mutex> lk(m_pool_mtx);
                m_size[p] = (size_t) size;
                return p;
        }

        void free_out_buf(char *buf) override
        {
                if (buf == nullptr) {
                        return;
                }
                std::lock_guard<std::mutex> lk(m_pool_mtx);
                auto it = m_size.find(buf);
                if (it == m_size.end()) {
                        return; // not ours
                }
                if ((int) m_free.size() < kMaxPooled) {
                        m_free.emplace(it->second, buf);
                } else {
                        m_size.erase(it);
                        ug_hip_free_host(buf);
                }
        }

        char *decode_frame(char *received, int buf_size, int *frame_size, std::map<int, int> valid_data) override
        {
                std::lock_guard<std::mutex> lk(m_code_mtx);
                *frame_size = 0;
                const int n = param_k + param_m;
                const int ps = buf_size / n;
                packet_size = ps;
                if (!ready()) {
                        return received + LDGM_session::HEADER_SIZE;
                }
                mark_received(valid_data, ps, n);
                for (int i = 0; i < param_k; ++i) {
                        if (!m_rx[i]) {
                                memset(received + (size_t) i * ps, 0, ps); // as LDGM_session_cpu::decode_frame does
                        }
                }
                int all_known = 0;
                if (ug_hip_ldgm_decode_host(m_session, received, ps, m_rx.data(), nullptr, &all_known, m_stream) != UG_HIP_SUCCESS) {
                        MSG(ERROR, "decode: %s\n", ug_hip_last_error_string());
                        return received + LDGM_session::HEADER_SIZE;
                }
                if (all_known) {
                        uint32_t fs = 0;
                        memcpy(&fs, received, sizeof fs);
                        *frame_size = (int) fs;
                }
                return received + LDGM_session::HEADER_SIZE;
        }

private:
        /// the coder for the current matrix (set_pcMatrix runs after construction, ldgm.cpp:set_params)
        bool ready()
        {
                if (pcm == nullptr) {
                        MSG(ERROR, "no parity-check matrix\n");
                        return false;
                }
                if (m_session != nullptr && m_pcm == pcm && m_k == param_k && m_m == param_m) {
                        return true;
                }
                ug_hip_ldgm_destroy(m_session);
                m_session = nullptr;
                if (m_stream == nullptr) {
                        if (ug_hip_set_device(m_device) != UG_HIP_SUCCESS || ug_hip_stream_create(&m_stream) != UG_HIP_SUCCESS) {
                                MSG(ERROR, "cannot use HIP device %d: %s\n", m_device, ug_hip_last_error_string());
                                m_stream = nullptr;
                                return false;
                        }
                }
                if (ug_hip_ldgm_create(m_device, param_k, param_m, pcm, max_row_weight + 2, &m_session) != UG_HIP_SUCCESS) {
                        MSG(ERROR, "LDGM k=%d m=%d on device %d: %s\n", (int) param_k, (int) param_m, m_device, ug_hip_last_error_string());
                        return false;
                }
                m_pcm = pcm;
                m_k = param_k;
                m_m = param_m;
                return true;
        }

        /// LDGM_session_cpu::decode_frame's rule (ldgm-session-cpu.cpp:316-380): entries whose end meets the next one's start merge, and
        /// packet i counts as received when the last merged interval starting at or before i * ps reaches (i + 1) * ps.  (The reference's
        /// merge loop reads the entry after the last one -- end() -- before it stops; this one stops at the last.)
        void mark_received(const std::map<int, int> &valid, int ps, int n)
        {
                std::vector<std::pair<long long, long long>> merged;
                for (auto it = valid.begin(); it != valid.end();) {
                        long long start = it->first, len = it->second;
                        for (++it; it != valid.end() && start + len == it->first; ++it) {
                                len += it->second;
                        }
                        merged.emplace_back(start, len);
                }
                m_rx.assign(n, 0);
                size_t j = 0; // merged intervals starting at or before the packet: [0, j)
                for (int i = 0; i < n; ++i) {
                        const long long off = (long long) i * ps;
                        while (j < merged.size() && merged[j].first <= off) {
                                ++j;
                        }
                        m_rx[i] = j > 0 && merged[j - 1].first + merged[j - 1].second >= off + ps;
                }
        }

        int m_device = 0;
        ug_hip_ldgm *m_session = nullptr;
        ug_hip_stream_t m_stream = nullptr;
        const int *m_pcm = nullptr;
        int m_k = 0, m_m = 0;
        std::vector<uint8_t> m_rx;
        std::mutex m_code_mtx;
        std::mutex m_pool_mtx;
        std::multimap<size_t, void *> m_free; // capacity -> free pinned buffer
        std::map<void *, size_t> m_size;       // every pinned buffer of the pool, out or free -> capacity
};

/* ldgm.cpp:223-231 takes the registered pointer as `LDGM_session_gpu *(*)()` and converts what it returns to `LDGM_session *` at once
 * (unique_ptr<LDGM_session>(loader())).  LDGM_session_gpu derives from LDGM_session alone and not virtually, so that conversion keeps the
 * address as it is; this function returns the LDGM_session subobject of its session, which is exactly the pointer the conversion must
 * produce.  Both types are plain object pointers returned the same way, and nothing ever uses the pointer as an LDGM_session_gpu. */
LDGM_session *new_ldgm_session_mi355x()
{
        return new LDGM_session_mi355x();
}

} // namespace

REGISTER_MODULE(ldgm_gpu, reinterpret_cast<const void *>(new_ldgm_session_mi355x), LIBRARY_CLASS_UNDEFINED, LDGM_GPU_API_VERSION);
