/* Channel slice and channel shuffle through the C ABI, plain C99 against include/f8net.h (see examples/host_demo.c for the build line).
 *
 * Records three graphs with f8_net_slice / f8_net_channel_shuffle, finalizes each (planning needs no GPU), prints the plans and destroys the handles:
 *   unit     a ShuffleNet-V2 stride-1 unit: split 58 / 58, 1x1 on the right half, concat, shuffle 2
 *            -> two slice_i8: launches and one concat+shuffle2_i8: launch (the concat emits none)
 *   unequal  concat(64, 32) -> shuffle 2: group i is not operand i               -> concat_i8: then shuffle2_i8:
 *   output   a shuffle by 3 of 24 channels that is the network output           -> shuffle3_i32:
 * and walks the refusals of both entry points.  tests/test_chanmap_plan.py builds the library's host code with AddressSanitizer and
 * UndefinedBehaviorSanitizer and runs this program against it. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "f8net.h"

#define CHECK(x) do { int rc_ = (x); if (rc_ < 0) { fprintf(stderr, "%s failed: %s\n", #x, f8_last_error()); return 1; } } while (0)
#define EXPECT(x, code) do { int rc_ = (x); if (rc_ != (code)) { fprintf(stderr, "%s: status %d, expected %d\n", #x, rc_, (code)); return 1; } } while (0)

static int32_t wbuf[128 * 128];

static int conv(f8_net* net, int src, int cin, int cout, int w_fl, int in_fl, int sgn, int quant, int relu) {
    f8_conv_desc d;
    int i;
    memset(&d, 0, sizeof d);
    d.cin = cin; d.cout = cout; d.kernel = 1; d.stride = 1; d.pad = 0; d.groups = 1;
    d.weight_fl = w_fl; d.input_fl = in_fl; d.input_signed = sgn; d.quant_input = quant; d.relu = relu;
    for (i = 0; i < cin * cout; ++i) wbuf[i] = (i * 7 + cout) % 11 - 5;
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
    EXPECT(f8_net_slice(net, out, 0, 1), F8_ERR_STATE);
    EXPECT(f8_net_channel_shuffle(net, out, 2), F8_ERR_STATE);
    f8_net_destroy(net);
    return 0;
}

int main(void) {
    int t[2], x, src, left, right, cat, k;
    f8_net* net;

    net = f8_net_create();                                   /* unit */
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 8, 7, 7, 8));
    CHECK(src = conv(net, x, 8, 116, 5, 8, 0, 0, 1));
    EXPECT(f8_net_slice(net, 99, 0, 1), F8_ERR_INVALID);
    EXPECT(f8_net_slice(net, src, -1, 4), F8_ERR_INVALID);
    EXPECT(f8_net_slice(net, src, 0, 0), F8_ERR_INVALID);
    EXPECT(f8_net_slice(net, src, 100, 17), F8_ERR_INVALID);
    EXPECT(f8_net_slice(net, src, 0, 116), F8_ERR_INVALID);              /* the whole tensor */
    EXPECT(f8_net_channel_shuffle(net, -1, 2), F8_ERR_INVALID);
    EXPECT(f8_net_channel_shuffle(net, src, 1), F8_ERR_INVALID);
    EXPECT(f8_net_channel_shuffle(net, src, 3), F8_ERR_INVALID);         /* 3 does not divide 116 */
    EXPECT(f8_net_channel_shuffle(net, src, 116), F8_ERR_INVALID);       /* the identity */
    EXPECT(f8_net_channel_shuffle(net, src, 29), F8_ERR_UNSUPPORTED);    /* more than F8_MAX_CONCAT groups */
    CHECK(left = f8_net_slice(net, src, 0, 58));
    CHECK(right = f8_net_slice(net, src, 58, 58));
    t[0] = left;
    CHECK(t[1] = conv(net, right, 58, 58, 0, 4, 0, 1, 1));              /* fraclen 4 next to the left half's 13 */
    CHECK(cat = f8_net_concat(net, t, 2));
    CHECK(k = f8_net_channel_shuffle(net, cat, 2));
    CHECK(k = conv(net, k, 116, 32, 6, 4, 0, 1, 0));
    if (finish(net, k, "unit")) return 1;

    net = f8_net_create();                                   /* unequal */
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 8, 7, 7, 8));
    CHECK(t[0] = conv(net, x, 8, 64, 5, 8, 0, 0, 1));
    CHECK(t[1] = conv(net, x, 8, 32, 5, 8, 0, 0, 1));
    CHECK(cat = f8_net_concat(net, t, 2));
    CHECK(k = f8_net_channel_shuffle(net, cat, 2));
    CHECK(k = conv(net, k, 96, 32, 6, 4, 0, 1, 0));
    if (finish(net, k, "unequal")) return 1;

    net = f8_net_create();                                   /* output */
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 8, 9, 11, 8));
    CHECK(src = conv(net, x, 8, 24, 5, 8, 0, 0, 0));
    CHECK(k = f8_net_channel_shuffle(net, src, 3));
    if (finish(net, k, "output")) return 1;
    printf("ok\n");
    return 0;
}
