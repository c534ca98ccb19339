/* A net with two outputs from plain C99 (include/f8net.h): 3x3 conv + ReLU -> 1x1 conv, joined with the first conv's output.
 * Output 0 is the join (int32), output 1 the first conv's result (float32).
 *
 *   gcc -std=c99 -Wall -Iinclude examples/host_outputs.c -Lf8net_amd -lf8net -Wl,-rpath,$PWD/f8net_amd -o build/host_outputs
 *
 * Finalizes the net (planning needs no GPU), prints the plan and f8_net_output_info of every output.  A run hands the buffers of
 * outputs 1 .. over before EVERY call:
 *
 *   void* bufs[1] = { features_dev };                       // float32 [N, 32, 8, 8]
 *   f8_net_set_output_buffers(net, bufs, 1);
 *   f8_net_run(net, input_dev, join_dev, N, stream);        // join_dev: int32 [N, 32 * 8 * 8]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "f8net.h"

#define CHECK(x) do { int rc_ = (x); if (rc_ < 0) { fprintf(stderr, "%s failed: %s\n", #x, f8_last_error()); return 1; } } while (0)

int main(void) {
    enum { C = 32, H = 8, W = 8, N = 2 };
    static int32_t w1[C * C * 9], w2[C * C], b1[C], b2[C];
    for (int i = 0; i < C * C * 9; ++i) w1[i] = (i * 7) % 11 - 5;
    for (int i = 0; i < C * C; ++i) w2[i] = (i * 5) % 9 - 4;
    for (int i = 0; i < C; ++i) { b1[i] = 100 * i; b2[i] = -50 * i; }

    f8_net* net = f8_net_create();
    if (!net) return 1;
    int x = f8_net_input(net, C, H, W, /*fraclen*/ 8);
    CHECK(x);
    f8_conv_desc d1; memset(&d1, 0, sizeof d1);
    d1.cin = C; d1.cout = C; d1.kernel = 3; d1.stride = 1; d1.pad = 1; d1.groups = 1;
    d1.weight_fl = 5; d1.input_fl = 6; d1.input_signed = 0; d1.quant_input = 1; d1.relu = 1;
    int t1 = f8_net_conv(net, x, &d1, w1, b1);
    CHECK(t1);
    f8_conv_desc d2 = d1;
    d2.kernel = 1; d2.pad = 0; d2.weight_fl = 6; d2.input_fl = 5; d2.relu = 0;
    int t2 = f8_net_conv(net, t1, &d2, w2, b2);
    CHECK(t2);
    int t3 = f8_net_add(net, t2, t1, /*relu*/ 1);
    CHECK(t3);
    int k0 = f8_net_output(net, t3, /*as_float*/ 0);
    CHECK(k0);
    int k1 = f8_net_output(net, t1, /*as_float*/ 1);
    CHECK(k1);
    printf("output indices %d %d\n", k0, k1);
    if (f8_net_output(net, t1, 0) != F8_ERR_INVALID) { fprintf(stderr, "a tensor was accepted as an output twice\n"); return 1; }
    CHECK(f8_net_finalize(net, N));
    size_t need = f8_net_describe(net, NULL, 0);
    char* plan = (char*)malloc(need);
    f8_net_describe(net, plan, need);
    printf("%s", plan);
    free(plan);
    for (int k = 0; k < f8_net_num_outputs(net); ++k) {
        int c, h, w, fl, as_float;
        CHECK(f8_net_output_info(net, k, &c, &h, &w, &fl, &as_float));
        printf("output %d: %d x %d x %d fraclen %d %s\n", k, c, h, w, fl, as_float ? "float32" : "int32");
    }
    if (f8_net_set_output_buffers(net, NULL, 0) != F8_ERR_INVALID) { fprintf(stderr, "0 buffers were accepted for one further output\n"); return 1; }
    f8_net_destroy(net);
    return 0;
}
