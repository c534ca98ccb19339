/* Windowed average pooling through the C ABI, plain C99 against include/f8net.h (see examples/host_demo.c for the build line).
 *
 * Records, finalizes (planning needs no GPU), prints the plan and destroys the handle:
 *   a DenseNet transition   conv 3x3 of the input (64 channels, 24 x 24) -> 1x1 to 32 -> average 2x2 / 2 (12 x 12, an exact average at fraclen + 2)
 *   a PSP pyramid           feat = conv 3x3 of the pooled map (64 channels); per bin count 1 / 2 / 3 / 6: the map averaged over (12 / bins)-square
 *                           windows -> 1x1 to 16 channels -> nearest upsample back to 12 x 12; concat(feat, the four branches) -> 1x1 classifier
 * Bin 1 is the global window: f8_net_avgpool_window records the node of f8_net_avgpool_sum and the plan names it `avgpool_sum:`; the others
 * plan `sumpool6x6s6:`, `sumpool4x4s4:`, `sumpool2x2s2:`.  Then it walks every refusal of f8_net_avgpool_window.  The library's host code is built
 * with AddressSanitizer and UndefinedBehaviorSanitizer and linked with this file into a stand-alone program. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "f8net.h"

#define CHECK(x) do { int rc_ = (x); if (rc_ < 0) { fprintf(stderr, "%s failed: %s\n", #x, f8_last_error()); return 1; } } while (0)
#define EXPECT(x, code) do { int rc_ = (x); if (rc_ != (code)) { fprintf(stderr, "%s: status %d, expected %d\n", #x, rc_, (code)); return 1; } } while (0)

static int32_t wbuf[128 * 64 * 9];

static int conv(f8_net* net, int src, int cin, int cout, int k, int w_fl, int in_fl, int quant, int relu) {
    f8_conv_desc d;
    int i;
    memset(&d, 0, sizeof d);
    d.cin = cin; d.cout = cout; d.kernel = k; d.stride = 1; d.pad = k / 2; d.groups = 1;
    d.weight_fl = w_fl; d.input_fl = in_fl; d.input_signed = 0; d.quant_input = quant; d.relu = relu;
    for (i = 0; i < cin * cout * k * k; ++i) wbuf[i] = (i * 7 + cout) % 11 - 5;
    return f8_net_conv(net, src, &d, wbuf, NULL);
}

/* round(log2(k * k)): FXQAvgPool2d(k).shiftnum */
static int pool_shift(int k) {
    int s = 0;
    while ((1 << (s + 1)) * (1 << (s + 1)) <= 2 * k * k * k * k) ++s;      /* 2^(2 (s + 1)) <= 2 k^4  <=>  s + 1 <= log2(k^2) + 1 / 2 */
    return s;
}

int main(void) {
    static const int bins[4] = {1, 2, 3, 6};
    int x, c1, t, tp, feat, cat, cls, srcs[5], b, C, H, W, fl, as_float;
    size_t need;
    char* plan;
    f8_net* net = f8_net_create();
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 8, 24, 24, 8));
    CHECK(c1 = conv(net, x, 8, 64, 3, 5, 8, 0, 1));
    CHECK(t = conv(net, c1, 64, 32, 1, 5, 4, 1, 0));
    /* refusals */
    EXPECT(f8_net_avgpool_window(NULL, t, 2, 2, 0, 2), F8_ERR_INVALID);
    EXPECT(f8_net_avgpool_window(net, 99, 2, 2, 0, 2), F8_ERR_INVALID);
    EXPECT(f8_net_avgpool_window(net, -1, 2, 2, 0, 2), F8_ERR_INVALID);
    EXPECT(f8_net_avgpool_window(net, t, 0, 2, 0, 2), F8_ERR_INVALID);
    EXPECT(f8_net_avgpool_window(net, t, 2, 0, 0, 2), F8_ERR_INVALID);
    EXPECT(f8_net_avgpool_window(net, t, 2, 2, -1, 2), F8_ERR_INVALID);
    EXPECT(f8_net_avgpool_window(net, t, 3, 1, 2, 3), F8_ERR_INVALID);       /* 2 pad > kernel */
    EXPECT(f8_net_avgpool_window(net, t, 1, 1, 0, 0), F8_ERR_INVALID);       /* the identity */
    EXPECT(f8_net_avgpool_window(net, t, 25, 1, 0, 9), F8_ERR_INVALID);      /* P < 1 */
    EXPECT(f8_net_avgpool_window(net, t, 2, 2, 0, -1), F8_ERR_INVALID);
    EXPECT(f8_net_avgpool_window(net, t, 2, 2, 0, 24), F8_ERR_INVALID);      /* fraclen 9 + 24 > 32 */
    EXPECT(f8_net_avgpool_window(net, t, 65, 1, 32, 12), F8_ERR_UNSUPPORTED);
    EXPECT(f8_net_avgpool_window(net, t, 2, 65, 0, 2), F8_ERR_UNSUPPORTED);
    /* the transition */
    CHECK(tp = f8_net_avgpool_window(net, t, 2, 2, 0, pool_shift(2)));
    CHECK(f8_net_set_label(net, tp, "transition.pool"));
    CHECK(f8_net_tensor_info(net, tp, &C, &H, &W, &fl));
    if (C != 32 || H != 12 || W != 12 || fl != 9 + 2) { fprintf(stderr, "transition is %d x %d x %d at fraclen %d\n", C, H, W, fl); return 1; }
    /* the pyramid */
    CHECK(feat = conv(net, tp, 32, 64, 3, 5, 4, 1, 1));
    srcs[0] = feat;
    for (b = 0; b < 4; ++b) {
        char name[32];
        const int k = H / bins[b];
        int p, u;
        CHECK(p = f8_net_avgpool_window(net, feat, k, k, 0, pool_shift(k)));
        sprintf(name, "psp.pool%d", bins[b]);
        CHECK(f8_net_set_label(net, p, name));
        CHECK(p = conv(net, p, 64, 16, 1, 5, 4, 1, 1));
        CHECK(u = f8_net_upsample(net, p, F8_UP_NEAREST, k, k));
        sprintf(name, "psp.up%d", bins[b]);
        CHECK(f8_net_set_label(net, u, name));
        srcs[1 + b] = u;
    }
    CHECK(cat = f8_net_concat(net, srcs, 5));
    CHECK(f8_net_set_label(net, cat, "psp.cat"));
    CHECK(cls = conv(net, cat, 128, 5, 1, 5, 4, 1, 0));
    CHECK(f8_net_output(net, cls, 0));
    CHECK(f8_net_finalize(net, 3));
    CHECK(f8_net_output_info(net, 0, &C, &H, &W, &fl, &as_float));
    if (C != 5 || H != 12 || W != 12 || fl != 9) { fprintf(stderr, "output is %d x %d x %d at fraclen %d\n", C, H, W, fl); return 1; }
    need = f8_net_describe(net, NULL, 0);
    plan = (char*)malloc(need);
    if (!plan) return 1;
    f8_net_describe(net, plan, need);
    printf("== transition + psp: %d launches, output %d x %d x %d at fraclen %d\n%s", f8_net_num_launches(net), C, H, W, fl, plan);
    free(plan);
    EXPECT(f8_net_avgpool_window(net, t, 2, 2, 0, 2), F8_ERR_STATE);
    f8_net_destroy(net);
    printf("ok\n");
    return 0;
}
