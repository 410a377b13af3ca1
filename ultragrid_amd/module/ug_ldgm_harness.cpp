/**
 * @file ug_ldgm_harness.cpp
 * Drives the reference's own `ldgm` FEC class (src/rtp/ldgm.cpp) -- with its CPU session, or, under UG_PARAM=ldgm-device=GPU, with
 * whatever registered "ldgm_gpu" (here: ldgm_gpu_mi355x.cpp, linked in) -- through the calls the sender and the receiver make.
 *
 *   ug_ldgm_harness encode <k> <m> <c> <seed> <payload file> <out file>
 *       one tile of the payload through ldgm::encode_video_frame; writes the tile's FEC buffer, prints "symbol_size=<ps> len=<bytes>"
 *   ug_ldgm_harness decode <k> <m> <c> <seed> <buffer file> <mask file> <out file>
 *       ldgm::decode of the buffer with the packets whose mask byte is 0 missing (valid_data = one entry per received packet, as the
 *       receiver's packet map holds them); writes the int32 out_len, then the k * ps data bytes after decoding; prints "ok=<0|1> len=<n>"
 *   ug_ldgm_harness time <k> <m> <c> <seed> <payload bytes> <loss %> <iterations>
 *       mean call time of encode_video_frame and of decode with <loss %> random losses, one thread: "encode_ms=.. decode_ms=.."
 *
 * UG_PARAM=<k>=<v>[,...] answers get_commandline_param (ldgm-device, mi355x-device), as `uv --param` would.
 * UG_LDGM_MATRIX_DIR=<dir>: where the matrices go.  ldgm::set_params writes them to /var/tmp/ultragrid-<uid>/; the harness is linked with
 * --wrap for mkdir / stat / fopen and sends paths under that directory to <dir> instead (a machine need not have a writable /var/tmp).
 */
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <sys/stat.h>
#include <vector>

#include "rtp/ldgm.hpp"
#include "types.h"
#include "video_frame.h"

extern "C" {
char *uv_argv[] = {(char *) "ug_ldgm_harness", nullptr};

const char *get_commandline_param(const char *key)
{
        static char vals[8][128];
        static int slot;
        const char *p = getenv("UG_PARAM");
        const size_t kl = strlen(key);
        while (p != nullptr && *p != '\0') {
                const char *end = strchr(p, ',');
                const size_t len = end ? (size_t) (end - p) : strlen(p);
                if (len >= kl && strncmp(p, key, kl) == 0 && (len == kl || p[kl] == '=')) {
                        char *v = vals[slot++ % 8];
                        snprintf(v, sizeof vals[0], "%.*s", len > kl ? (int) (len - kl - 1) : 0, p + kl + (len > kl ? 1 : 0));
                        return v;
                }
                p = end ? end + 1 : nullptr;
        }
        return nullptr;
}

void register_param(const char *, const char *) {}
bool tok_in_argv(char **, const char *) { return false; }

// the FEC layer treats the video header as opaque bytes: a fixed pattern stands in for transmit.c's format_video_header
void format_video_header(const struct video_frame *, int tile_idx, int buffer_idx, uint32_t *hdr)
{
        for (int i = 0; i < 6; ++i) {
                hdr[i] = 0x01020304u * (uint32_t) (i + 1) + (uint32_t) tile_idx + (uint32_t) buffer_idx;
        }
}

// --- the matrix directory (see the file comment) ---
int __real_mkdir(const char *, mode_t);
int __real_stat(const char *, struct stat *);
FILE *__real_fopen(const char *, const char *);

static const char *redirect(const char *path, std::string &buf)
{
        const char *dir = getenv("UG_LDGM_MATRIX_DIR");
        const char *pre = "/var/tmp/ultragrid-";
        if (dir == nullptr || *dir == '\0' || strncmp(path, pre, strlen(pre)) != 0) {
                return path;
        }
        const char *rest = strchr(path + strlen(pre), '/'); // after "<uid>"
        buf = std::string(dir) + (rest ? rest : "/");
        return buf.c_str();
}
int __wrap_mkdir(const char *path, mode_t mode)
{
        std::string b;
        return __real_mkdir(redirect(path, b), mode);
}
int __wrap_stat(const char *path, struct stat *st)
{
        std::string b;
        return __real_stat(redirect(path, b), st);
}
FILE *__wrap_fopen(const char *path, const char *mode)
{
        std::string b;
        return __real_fopen(redirect(path, b), mode);
}
}

static std::vector<char> slurp(const char *p)
{
        std::vector<char> v;
        FILE *f = fopen(p, "rb");
        if (!f) {
                perror(p);
                exit(2);
        }
        char b[65536];
        size_t n;
        while ((n = fread(b, 1, sizeof b, f)) > 0) {
                v.insert(v.end(), b, b + n);
        }
        fclose(f);
        return v;
}

static void dump(const char *p, const void *d, size_t n)
{
        FILE *f = fopen(p, "wb");
        if (!f || fwrite(d, 1, n, f) != n) {
                perror(p);
                exit(2);
        }
        fclose(f);
}

static struct video_frame *tile_frame(std::vector<char> &payload)
{
        struct video_desc desc{};
        desc.width = 1920;
        desc.height = 1080;
        desc.color_spec = UYVY;
        desc.interlacing = PROGRESSIVE;
        desc.fps = 30;
        desc.tile_count = 1;
        struct video_frame *f = vf_alloc_desc(desc);
        f->tiles[0].data = payload.data();
        f->tiles[0].data_len = (unsigned) payload.size();
        return f;
}

static std::map<int, int> valid_from_mask(const std::vector<char> &mask, int ps)
{
        std::map<int, int> valid;
        for (size_t i = 0; i < mask.size(); ++i) {
                if (mask[i]) {
                        valid[(int) i * ps] = ps;
                }
        }
        return valid;
}

int main(int argc, char **argv)
{
        if (argc < 6) {
                fprintf(stderr, "usage: see ug_ldgm_harness.cpp\n");
                return 2;
        }
        const std::string mode = argv[1];
        const unsigned k = atoi(argv[2]), m = atoi(argv[3]), c = atoi(argv[4]), seed = atoi(argv[5]);
        try {
                ldgm coder(k, m, c, seed);
                if (mode == "encode" && argc == 8) {
                        std::vector<char> payload = slurp(argv[6]);
                        struct video_frame *in = tile_frame(payload);
                        struct video_frame *out = coder.encode_video_frame(in);
                        if (out->tiles[0].data == nullptr) {
                                fprintf(stderr, "encode_video_frame: no buffer\n");
                                return 1;
                        }
                        dump(argv[7], out->tiles[0].data, out->tiles[0].data_len);
                        printf("symbol_size=%d len=%u\n", (int) out->fec_params.symbol_size, out->tiles[0].data_len);
                        vf_free(out);
                        in->tiles[0].data = nullptr;
                        vf_free(in);
                        return 0;
                }
                if (mode == "decode" && argc == 9) {
                        std::vector<char> buf = slurp(argv[6]), mask = slurp(argv[7]);
                        if (mask.size() != k + m) {
                                fprintf(stderr, "mask must hold k + m bytes\n");
                                return 2;
                        }
                        const int ps = (int) buf.size() / (int) (k + m);
                        char *out = nullptr;
                        int out_len = 0;
                        const bool ok = coder.decode(buf.data(), (int) buf.size(), &out, &out_len, valid_from_mask(mask, ps));
                        std::vector<char> res(sizeof(int) + (size_t) k * ps);
                        memcpy(res.data(), &out_len, sizeof(int));
                        memcpy(res.data() + sizeof(int), buf.data(), (size_t) k * ps);
                        dump(argv[8], res.data(), res.size());
                        printf("ok=%d len=%d\n", ok ? 1 : 0, out_len);
                        return 0;
                }
                if (mode == "time" && argc == 9) {
                        const size_t bytes = strtoull(argv[6], nullptr, 10);
                        const double loss = atof(argv[7]) / 100.0;
                        const int iters = atoi(argv[8]);
                        std::mt19937 rng(1);
                        std::vector<char> payload(bytes);
                        for (auto &b : payload) {
                                b = (char) rng();
                        }
                        struct video_frame *in = tile_frame(payload);
                        struct video_frame *enc = coder.encode_video_frame(in); // warm-up, and the buffer decode starts from
                        std::vector<char> clean(enc->tiles[0].data, enc->tiles[0].data + enc->tiles[0].data_len);
                        vf_free(enc);
                        using clk = std::chrono::steady_clock;
                        auto t0 = clk::now();
                        for (int i = 0; i < iters; ++i) {
                                vf_free(coder.encode_video_frame(in));
                        }
                        const double enc_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count() / iters;
                        const int ps = (int) clean.size() / (int) (k + m);
                        std::vector<char> mask(k + m);
                        std::uniform_real_distribution<double> u(0.0, 1.0);
                        for (auto &x : mask) {
                                x = u(rng) >= loss;
                        }
                        const std::map<int, int> valid = valid_from_mask(mask, ps);
                        std::vector<char> work(clean.size());
                        double dec_ms = 0;
                        int ok = 0;
                        for (int i = 0; i <= iters; ++i) {
                                memcpy(work.data(), clean.data(), clean.size());
                                char *out = nullptr;
                                int out_len = 0;
                                auto t1 = clk::now();
                                const bool r = coder.decode(work.data(), (int) work.size(), &out, &out_len, valid);
                                if (i > 0) { // the first call is a warm-up
                                        dec_ms += std::chrono::duration<double, std::milli>(clk::now() - t1).count();
                                        ok += r;
                                }
                        }
                        printf("encode_ms=%.4f decode_ms=%.4f decoded=%d/%d ps=%d\n", enc_ms, dec_ms / iters, ok, iters, ps);
                        in->tiles[0].data = nullptr;
                        vf_free(in);
                        return 0;
                }
        } catch (std::string const &e) {
                fprintf(stderr, "ldgm: %s\n", e.c_str());
                return 1;
        } catch (int e) {
                fprintf(stderr, "ldgm: error %d\n", e);
                return 1;
        }
        fprintf(stderr, "usage: see ug_ldgm_harness.cpp\n");
        return 2;
}
