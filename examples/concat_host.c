/* Channel concatenation through the C ABI, plain C99 against include/f8net.h (see examples/host_demo.c for the build line).
 *
 * Records three graphs with f8_net_concat, finalizes each (planning needs no GPU), prints the plans and destroys the handles:
 *   bytes    3 + 5 + 9 channels at byte offsets, one int8 reader                 -> concat_i8: on the general kernel instance
 *   raw      the network input itself next to a conv of it, fraclens 2 and 9     -> concat_i32: (nothing bounds the input)
 *   nested   DenseNet growth, 64 + 4 x 32 channels, each 3x3 reading the running concatenation -> four concat_i8: launches
 * and walks the refusals of f8_net_concat.  tests/test_concat_plan.py builds the library's host code with AddressSanitizer and
 * UndefinedBehaviorSanitizer and runs this program against it. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "f8net.h"

#define CHECK(x) do { int rc_ = (x); if (rc_ < 0) { fprintf(stderr, "%s failed: %s\n", #x, f8_last_error()); return 1; } } while (0)
#define EXPECT(x, code) do { int rc_ = (x); if (rc_ != (code)) { fprintf(stderr, "%s: status %d, expected %d\n", #x, rc_, (code)); return 1; } } while (0)

static int32_t wbuf[160 * 32 * 9];

static int conv(f8_net* net, int src, int cin, int cout, int k, int w_fl, int in_fl, int sgn, int quant, int relu) {
    f8_conv_desc d;
    int i;
    memset(&d, 0, sizeof d);
    d.cin = cin; d.cout = cout; d.kernel = k; d.stride = 1; d.pad = k / 2; d.groups = 1;
    d.weight_fl = w_fl; d.input_fl = in_fl; d.input_signed = sgn; d.quant_input = quant; d.relu = relu;
    for (i = 0; i < cin * cout * k * k; ++i) wbuf[i] = (i * 7 + cout) % 11 - 5;
    return f8_net_conv(net, src, &d, wbuf, NULL);
}

static int finish(f8_net* net, int out, const char* what) {
    size_t need;
    char* plan;
    CHECK(f8_net_output(net, out, 0));
    CHECK(f8_net_finalize(net, 3));
    need = f8_net_describe(net, NULL, 0);
    plan = (char*)malloc(need);
    if (!plan) return 1;
    f8_net_describe(net, plan, need);
    printf("== %s: %d launches\n%s", what, f8_net_num_launches(net), plan);
    free(plan);
    EXPECT(f8_net_concat(net, &out, 2), F8_ERR_STATE);
    f8_net_destroy(net);
    return 0;
}

int main(void) {
    int t[F8_MAX_CONCAT + 1], x, cat, k;
    f8_net* net;

    net = f8_net_create();                                   /* bytes */
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 3, 5, 5, 8));
    CHECK(t[0] = conv(net, x, 3, 3, 1, 5, 8, 0, 0, 1));
    CHECK(t[1] = conv(net, x, 3, 5, 1, 5, 8, 0, 0, 1));
    CHECK(t[2] = conv(net, x, 3, 9, 1, 5, 8, 0, 0, 1));
    EXPECT(f8_net_concat(net, t, 1), F8_ERR_INVALID);
    EXPECT(f8_net_concat(net, NULL, 2), F8_ERR_INVALID);
    t[3] = 99;
    EXPECT(f8_net_concat(net, t, 4), F8_ERR_INVALID);
    t[3] = t[1];
    EXPECT(f8_net_concat(net, t, 4), F8_ERR_UNSUPPORTED);
    for (k = 3; k <= F8_MAX_CONCAT; ++k) t[k] = t[0];
    EXPECT(f8_net_concat(net, t, F8_MAX_CONCAT + 1), F8_ERR_UNSUPPORTED);
    CHECK(cat = f8_net_concat(net, t, 3));
    CHECK(k = conv(net, cat, 17, 32, 1, 6, 4, 0, 1, 0));
    if (finish(net, k, "bytes")) return 1;

    net = f8_net_create();                                   /* raw */
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 8, 6, 6, 2));
    t[0] = x;
    CHECK(t[1] = conv(net, x, 8, 24, 1, 9, 0, 1, 1, 0));
    CHECK(cat = f8_net_concat(net, t, 2));
    CHECK(k = conv(net, cat, 32, 32, 1, 6, 4, 1, 1, 0));
    if (finish(net, k, "raw")) return 1;

    net = f8_net_create();                                   /* nested */
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 8, 8, 8, 8));
    CHECK(t[0] = conv(net, x, 8, 64, 1, 5, 8, 0, 0, 1));
    for (k = 0; k < 4; ++k) {
        CHECK(t[1] = conv(net, t[0], 64 + 32 * k, 32, 3, 8 + (k & 1), 4 - (k & 1), 0, 1, 1));
        CHECK(t[0] = f8_net_concat(net, t, 2));
    }
    CHECK(k = conv(net, t[0], 192, 32, 1, 6, 4, 0, 1, 0));
    if (finish(net, k, "nested")) return 1;
    printf("ok\n");
    return 0;
}
