/* Upsampling through the C ABI, plain C99 against include/f8net.h (see examples/host_demo.c for the build line).
 *
 * Records a small FPN-style graph with f8_net_upsample, finalizes it (planning needs no GPU), prints the plan and destroys the handle:
 *   c3  = conv 3x3 of the input (64 channels, 16 x 16)        c4 = conv 3x3 / 2 of c3 (128 channels, 8 x 8)
 *   p4  = 1x1 of c4 to 32 channels                            p3 = 1x1 of c3 to 32 channels + nearest x2 of p4   (the top-down join)
 *   seg = bilinear x4 of a 1x1 classifier (5 classes) on p3, output 0 at 64 x 64;  p4 broadcast: avgpool_sum -> 1x1 -> nearest (8, 8), read by a conv
 * The nearest upsample in front of the join plans upsample_nearest_i32: (the join reads int32), the broadcast upsample_nearest_i8: (one int8
 * reader), the logits upsample_bilinear_i32:.  Then it walks the refusals of f8_net_upsample.  The library's host code is built with
 * AddressSanitizer and UndefinedBehaviorSanitizer and linked with this file into a stand-alone program. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "f8net.h"

#define CHECK(x) do { int rc_ = (x); if (rc_ < 0) { fprintf(stderr, "%s failed: %s\n", #x, f8_last_error()); return 1; } } while (0)
#define EXPECT(x, code) do { int rc_ = (x); if (rc_ != (code)) { fprintf(stderr, "%s: status %d, expected %d\n", #x, rc_, (code)); return 1; } } while (0)

static int32_t wbuf[128 * 64 * 9];

static int conv(f8_net* net, int src, int cin, int cout, int k, int stride, int w_fl, int in_fl, int quant, int relu) {
    f8_conv_desc d;
    int i;
    memset(&d, 0, sizeof d);
    d.cin = cin; d.cout = cout; d.kernel = k; d.stride = stride; d.pad = k / 2; d.groups = 1;
    d.weight_fl = w_fl; d.input_fl = in_fl; d.input_signed = 0; d.quant_input = quant; d.relu = relu;
    for (i = 0; i < cin * cout * k * k; ++i) wbuf[i] = (i * 7 + cout) % 11 - 5;
    return f8_net_conv(net, src, &d, wbuf, NULL);
}

int main(void) {
    int x, c3, c4, p4, p3, up, lat, cls, seg, pooled, bc, side, C, H, W, fl, as_float;
    size_t need;
    char* plan;
    f8_net* net = f8_net_create();
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 8, 16, 16, 8));
    CHECK(c3 = conv(net, x, 8, 64, 3, 1, 5, 8, 0, 1));
    CHECK(c4 = conv(net, c3, 64, 128, 3, 2, 5, 4, 1, 1));
    CHECK(p4 = conv(net, c4, 128, 32, 1, 1, 5, 4, 1, 0));
    /* refusals */
    EXPECT(f8_net_upsample(NULL, p4, F8_UP_NEAREST, 2, 2), F8_ERR_INVALID);
    EXPECT(f8_net_upsample(net, 99, F8_UP_NEAREST, 2, 2), F8_ERR_INVALID);
    EXPECT(f8_net_upsample(net, -1, F8_UP_NEAREST, 2, 2), F8_ERR_INVALID);
    EXPECT(f8_net_upsample(net, p4, F8_UP_NEAREST, 0, 2), F8_ERR_INVALID);
    EXPECT(f8_net_upsample(net, p4, F8_UP_NEAREST, 1, 1), F8_ERR_INVALID);
    EXPECT(f8_net_upsample(net, p4, 2, 2, 2), F8_ERR_INVALID);
    EXPECT(f8_net_upsample(net, p4, F8_UP_NEAREST, 257, 1), F8_ERR_UNSUPPORTED);
    EXPECT(f8_net_upsample(net, p4, F8_UP_BILINEAR, 2, 4), F8_ERR_UNSUPPORTED);
    EXPECT(f8_net_upsample(net, p4, F8_UP_BILINEAR, 3, 3), F8_ERR_UNSUPPORTED);
    EXPECT(f8_net_upsample(net, p4, F8_UP_BILINEAR, 32, 32), F8_ERR_UNSUPPORTED);
    /* the top-down join */
    CHECK(up = f8_net_upsample(net, p4, F8_UP_NEAREST, 2, 2));
    CHECK(f8_net_set_label(net, up, "p4.up"));
    CHECK(lat = conv(net, c3, 64, 32, 1, 1, 5, 4, 1, 0));
    CHECK(p3 = f8_net_add(net, up, lat, 0));
    /* the broadcast of a pooled vector, read by one conv; joined into p3 so that it is part of the output */
    CHECK(pooled = f8_net_avgpool_sum(net, c4, 6));
    CHECK(pooled = conv(net, pooled, 128, 32, 1, 1, 5, 4, 1, 1));
    CHECK(bc = f8_net_upsample(net, pooled, F8_UP_NEAREST, 16, 16));
    CHECK(f8_net_set_label(net, bc, "pool.bcast"));
    CHECK(side = conv(net, bc, 32, 32, 1, 1, 5, 4, 1, 0));
    CHECK(p3 = f8_net_add(net, p3, side, 1));
    /* logits back at four times the map */
    CHECK(cls = conv(net, p3, 32, 5, 1, 1, 5, 4, 1, 0));
    CHECK(seg = f8_net_upsample(net, cls, F8_UP_BILINEAR, 4, 4));
    CHECK(f8_net_set_label(net, seg, "seg"));
    CHECK(f8_net_output(net, seg, 0));
    CHECK(f8_net_finalize(net, 3));
    CHECK(f8_net_output_info(net, 0, &C, &H, &W, &fl, &as_float));
    if (C != 5 || H != 64 || W != 64 || fl != 9 + 6) { fprintf(stderr, "output is %d x %d x %d at fraclen %d\n", C, H, W, fl); return 1; }
    need = f8_net_describe(net, NULL, 0);
    plan = (char*)malloc(need);
    if (!plan) return 1;
    f8_net_describe(net, plan, need);
    printf("== fpn: %d launches, output %d x %d x %d at fraclen %d\n%s", f8_net_num_launches(net), C, H, W, fl, plan);
    free(plan);
    EXPECT(f8_net_upsample(net, p4, F8_UP_NEAREST, 2, 2), F8_ERR_STATE);
    f8_net_destroy(net);
    printf("ok\n");
    return 0;
}
