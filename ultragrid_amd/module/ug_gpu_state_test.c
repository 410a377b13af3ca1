/**
 * @file ug_gpu_state_test.c
 * mi355x_gpu_state.h without a GPU: the nine ug_hip_* functions the header calls are defined HERE (the prototypes of include/ug_mi355x.h), on
 * malloc, with a log of the calls and a switch that makes the n-th call of a kind fail -- the failure paths of the module states (a bad device
 * list, no stream, an allocation that fails half way, a sync that fails after a good launch) never run on a healthy GPU: no GPU test reaches them.
 * Links neither libug_mi355x.so nor the reference; built plain and with -fsanitize=address,undefined (module/Makefile), run by
 * tests/test_sanitizers.py.  Prints OK and exits 0 only if every check holds.
 */
#include <stdarg.h>

#define UG_HARNESS_NAME "ug_gpu_state_test"
#include "ug_harness_host.h"
#include "mi355x_gpu_state.h"

enum kind { SET_DEVICE, STREAM_CREATE, STREAM_DESTROY, STREAM_SYNC, MALLOC, FREE, MALLOC_HOST, FREE_HOST, KINDS };
static struct call {
        enum kind   kind;
        const void *ptr; ///< the stream or buffer of the call
        int         device;
} calls[64];
static int n_calls, seen[KINDS], fail_at[KINDS]; ///< fail_at[k] = n: the n-th call of kind k from now fails (0: none)
static int live_bufs[2], live_streams, messages;
static char last_message[256];

static int stand_in(enum kind k, const void *ptr, int device)
{
        if (n_calls < (int) (sizeof calls / sizeof calls[0])) calls[n_calls] = (struct call){ k, ptr, device };
        n_calls++;
        seen[k]++;
        return fail_at[k] > 0 && --fail_at[k] == 0 ? UG_HIP_ERUNTIME : UG_HIP_SUCCESS;
}
static int alloc(enum kind k, void **buffer, size_t size)
{
        if (stand_in(k, NULL, -1) != UG_HIP_SUCCESS) {
                return UG_HIP_ERUNTIME;
        }
        calls[n_calls - 1].ptr = *buffer = malloc(size);
        live_bufs[k == MALLOC_HOST]++;
        return UG_HIP_SUCCESS;
}
int ug_hip_set_device(int index) { return stand_in(SET_DEVICE, NULL, index); }
int ug_hip_malloc(void **buffer, size_t size) { return alloc(MALLOC, buffer, size); }
int ug_hip_malloc_host(void **buffer, size_t size) { return alloc(MALLOC_HOST, buffer, size); }
int ug_hip_free(void *buffer) { live_bufs[0]--; free(buffer); return stand_in(FREE, buffer, -1); }
int ug_hip_free_host(void *buffer) { live_bufs[1]--; free(buffer); return stand_in(FREE_HOST, buffer, -1); }
int ug_hip_stream_create(ug_hip_stream_t *stream)
{
        if (stand_in(STREAM_CREATE, NULL, -1) != UG_HIP_SUCCESS) {
                return UG_HIP_ERUNTIME;
        }
        *stream = malloc(1);
        live_streams++;
        return UG_HIP_SUCCESS;
}
int ug_hip_stream_destroy(ug_hip_stream_t stream) { live_streams--; free(stream); return stand_in(STREAM_DESTROY, stream, -1); }
int ug_hip_stream_sync(ug_hip_stream_t stream) { return stand_in(STREAM_SYNC, stream, -1); }
const char *ug_hip_last_error_string(void) { return "stand-in error"; }

void log_msg(int level, const char *format, ...)
{
        (void) level;
        va_list ap;
        va_start(ap, format);
        vsnprintf(last_message, sizeof last_message, format, ap);
        va_end(ap);
        messages++;
}

static int failures;
#define CHECK(cond) \
        do { \
                if (!(cond)) { \
                        printf("FAILED line %d: %s\n", __LINE__, #cond); \
                        failures++; \
                } \
        } while (0)
static void fresh(void)
{
        n_calls = messages = 0;
        memset(seen, 0, sizeof seen);
        memset(fail_at, 0, sizeof fail_at);
}
static bool said(const char *text) { return strstr(last_message, text) != NULL; }

static void test_open_close(void)
{
        unsigned counter = 0;
        struct mi355x_gpu g[3];
        static const int want[] = { 1, 3, 1 };
        setenv("UG_PARAM", "mi355x-device=1:3", 1);
        for (int i = 0; i < 3; i++) { // the listed devices in turn, the device set before the stream is made
                fresh();
                CHECK(mi355x_gpu_open(&g[i], &counter, "[test] "));
                CHECK(g[i].device == want[i] && g[i].stream != NULL && messages == 0);
                CHECK(n_calls == 2 && calls[0].kind == SET_DEVICE && calls[0].device == want[i] && calls[1].kind == STREAM_CREATE);
        }
        fresh();
        CHECK(mi355x_gpu_enter(&g[1]) && n_calls == 1 && calls[0].kind == SET_DEVICE && calls[0].device == 3);
        fail_at[SET_DEVICE] = 1;
        CHECK(!mi355x_gpu_enter(&g[1]) && messages == 1 && said("[test] cannot use HIP device 3: stand-in error"));
        const void *stream = g[1].stream;
        fresh(); // close: the device, the sync, the stream; a second close does nothing
        mi355x_gpu_close(&g[1]);
        CHECK(n_calls == 3 && calls[0].kind == SET_DEVICE && calls[0].device == 3 && calls[1].kind == STREAM_SYNC && calls[1].ptr == stream &&
              calls[2].kind == STREAM_DESTROY && calls[2].ptr == stream && g[1].stream == NULL);
        mi355x_gpu_close(&g[1]);
        CHECK(n_calls == 3);
        mi355x_gpu_close(&g[0]);
        mi355x_gpu_close(&g[2]);

        struct mi355x_gpu bad = { 0 };
        setenv("UG_PARAM", "mi355x-device=x", 1); // a malformed list: refused before any device call, and next_state_device has spoken
        fresh();
        CHECK(!mi355x_gpu_open(&bad, &counter, "[test] ") && bad.stream == NULL);
        CHECK(messages == 1 && said("expected <n>[:<n>...]"));
        mi355x_gpu_close(&bad);
        CHECK(n_calls == 0);

        setenv("UG_PARAM", "mi355x-device=2", 1);
        fresh();
        fail_at[STREAM_CREATE] = 1;
        CHECK(!mi355x_gpu_open(&bad, &counter, "[test] ") && bad.stream == NULL && messages == 1 && said("cannot use HIP device 2"));
        mi355x_gpu_close(&bad);
        CHECK(seen[STREAM_DESTROY] == 0 && seen[STREAM_SYNC] == 0);
        fresh();
        fail_at[SET_DEVICE] = 1;
        CHECK(!mi355x_gpu_open(&bad, &counter, "[test] ") && bad.stream == NULL && seen[STREAM_CREATE] == 0 && said("cannot use HIP device 2"));
}

static void test_reserve(bool pinned)
{
        const enum kind a = pinned ? MALLOC_HOST : MALLOC, f = pinned ? FREE_HOST : FREE;
        struct mi355x_buf b = { .pinned = pinned };
        fresh();
        mi355x_buf_release(&b); // an empty buf
        CHECK(n_calls == 0);
        CHECK(mi355x_buf_reserve(&b, 16) && n_calls == 1 && calls[0].kind == a && b.ptr != NULL && b.ptr == calls[0].ptr && b.cap == 16);
        const void *first = b.ptr;
        CHECK(mi355x_buf_reserve(&b, 8) && n_calls == 1 && b.ptr == first && b.cap == 16);
        CHECK(mi355x_buf_reserve(&b, 32) && n_calls == 3 && calls[1].kind == f && calls[1].ptr == first && calls[2].kind == a && b.ptr == calls[2].ptr && b.cap == 32);
        const void *second = b.ptr;
        fail_at[a] = 1;
        CHECK(!mi355x_buf_reserve(&b, 64) && b.ptr == NULL && b.cap == 0);
        CHECK(n_calls == 5 && calls[3].kind == f && calls[3].ptr == second && calls[4].kind == a && seen[f] == 2);
        CHECK(mi355x_buf_reserve(&b, 8) && n_calls == 6 && calls[5].kind == a && b.ptr != NULL && b.cap == 8);
        mi355x_buf_release(&b);
        CHECK(n_calls == 7 && calls[6].kind == f && b.ptr == NULL && b.cap == 0);
        mi355x_buf_release(&b);
        CHECK(n_calls == 7 && messages == 0);
        CHECK(seen[pinned ? MALLOC : MALLOC_HOST] == 0 && seen[pinned ? FREE : FREE_HOST] == 0); // only its own pair
}

static void test_finish(void)
{
        unsigned counter = 0;
        struct mi355x_gpu g;
        setenv("UG_PARAM", "mi355x-device=0", 1);
        CHECK(mi355x_gpu_open(&g, &counter, "[test] "));
        fresh();
        CHECK(!mi355x_gpu_finish(&g, false, "scale") && seen[STREAM_SYNC] == 1 && n_calls == 1 && messages == 1 && said("[test] scale failed: stand-in error"));
        fresh();
        CHECK(!mi355x_gpu_finish(&g, false, NULL) && seen[STREAM_SYNC] == 1 && messages == 0);
        fresh();
        fail_at[STREAM_SYNC] = 1;
        CHECK(!mi355x_gpu_finish(&g, true, "scale") && seen[STREAM_SYNC] == 1 && messages == 1 && said("[test] stream sync") && said("failed: stand-in error"));
        fresh();
        CHECK(mi355x_gpu_finish(&g, true, "scale") && seen[STREAM_SYNC] == 1 && calls[0].ptr == g.stream && messages == 0);
        mi355x_gpu_close(&g);
}

int main(void)
{
        test_open_close();
        test_reserve(false);
        test_reserve(true);
        test_finish();
        CHECK(live_bufs[0] == 0 && live_bufs[1] == 0 && live_streams == 0);
        if (failures == 0) printf("OK\n");
        return failures == 0 ? 0 : 1;
}
