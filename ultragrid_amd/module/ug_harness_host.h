/**
 * @file ug_harness_host.h
 * What host.cpp would provide, for the plain-C filter harnesses (ug_vopp_, ug_deint_, ug_cfilter_, ug_compose_harness.c) and ug_gpu_state_test.c (one copy; each harness is one translation unit and includes this once).  The
 * reference's tools/ug_stub.c answers NULL to every key; get_commandline_param here answers from what set_commandline_param stored, then from
 * UG_PARAM=<k>=<v>[,<k>=<v>...], which is what `uv --param ...` would hold (host.cpp:1090-1121).
 * The harness defines UG_HARNESS_NAME (uv_argv[0]) before the include.
 */
#ifndef UG_HARNESS_HOST_H
#define UG_HARNESS_HOST_H

#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

static char *uv_argv_store[] = { UG_HARNESS_NAME, NULL };
char **uv_argv = uv_argv_store;
static char set_keys[8][64], set_vals[8][128];
static int set_count;
void register_param(const char *param, const char *doc) { (void) param, (void) doc; }
bool tok_in_argv(char **argv, const char *tok) { (void) argv, (void) tok; return false; }
void set_commandline_param(const char *key, const char *val)
{
        if (set_count < 8) {
                snprintf(set_keys[set_count], sizeof set_keys[0], "%s", key);
                snprintf(set_vals[set_count++], sizeof set_vals[0], "%s", val);
        }
}
const char *get_commandline_param(const char *key)
{
        static char vals[8][128];
        static int slot;
        for (int i = 0; i < set_count; i++) {
                if (strcmp(set_keys[i], key) == 0) return set_vals[i];
        }
        const char *p = getenv("UG_PARAM");
        const size_t kl = strlen(key);
        while (p != NULL && *p != '\0') {
                const char *end = strchr(p, ',');
                const size_t len = end ? (size_t) (end - p) : strlen(p);
                if (len >= kl && strncmp(p, key, kl) == 0 && (len == kl || p[kl] == '=')) {
                        char *v = vals[slot++ % 8];
                        snprintf(v, sizeof vals[0], "%.*s", len > kl ? (int) (len - kl - 1) : 0, p + kl + (len > kl ? 1 : 0));
                        return v;
                }
                p = end ? end + 1 : NULL;
        }
        return NULL;
}

static inline double now_ms(void)
{
        struct timespec t;
        clock_gettime(CLOCK_MONOTONIC, &t);
        return (double) t.tv_sec * 1e3 + (double) t.tv_nsec / 1e6;
}

#endif /* UG_HARNESS_HOST_H */
