/* Depth-to-space and space-to-depth through the C ABI, plain C99 against include/f8net.h (see examples/host_demo.c for the build line).
 *
 * Records three graphs with f8_net_depth_to_space / f8_net_space_to_depth, finalizes each (planning needs no GPU), prints the plans and destroys the
 * handles:
 *   espcn    conv 1x1 to 27 -> depth_to_space 3 (CRD: torch's pixel_shuffle) as the network output          -> d2s3crd_i32:
 *   edsr     conv 1x1 to 64 -> depth_to_space 2 (CRD) -> conv: the shuffle's only reader is an int8 reader   -> d2s2crd_i8:
 *   stem     the input -> space_to_depth 4 (DCR: TResNet's stem) -> conv                                     -> s2d4dcr_i8:
 * and walks the refusals of both entry points.  tests/test_pixmap_plan.py builds the library's host code with AddressSanitizer and
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
    EXPECT(f8_net_depth_to_space(net, out, 2, F8_ORDER_CRD), F8_ERR_STATE);
    EXPECT(f8_net_space_to_depth(net, out, 2, F8_ORDER_DCR), F8_ERR_STATE);
    f8_net_destroy(net);
    return 0;
}

int main(void) {
    int x, src, k;
    f8_net* net;

    net = f8_net_create();                                   /* espcn */
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 8, 6, 5, 8));
    CHECK(src = conv(net, x, 8, 27, 5, 8, 0, 0, 0));
    EXPECT(f8_net_depth_to_space(net, 99, 3, F8_ORDER_CRD), F8_ERR_INVALID);
    EXPECT(f8_net_depth_to_space(net, -1, 3, F8_ORDER_CRD), F8_ERR_INVALID);
    EXPECT(f8_net_depth_to_space(net, src, 1, F8_ORDER_CRD), F8_ERR_INVALID);
    EXPECT(f8_net_depth_to_space(net, src, 3, 2), F8_ERR_INVALID);                /* no such order */
    EXPECT(f8_net_depth_to_space(net, src, 2, F8_ORDER_DCR), F8_ERR_INVALID);     /* 4 does not divide 27 */
    EXPECT(f8_net_depth_to_space(net, src, 17, F8_ORDER_DCR), F8_ERR_UNSUPPORTED);
    EXPECT(f8_net_space_to_depth(net, src, 2, F8_ORDER_CRD), F8_ERR_INVALID);     /* 2 divides 6 but not 5 */
    EXPECT(f8_net_space_to_depth(net, src, 0, F8_ORDER_CRD), F8_ERR_INVALID);
    EXPECT(f8_net_space_to_depth(net, src, 32, F8_ORDER_CRD), F8_ERR_UNSUPPORTED);
    EXPECT(f8_net_space_to_depth(NULL, src, 2, F8_ORDER_CRD), F8_ERR_INVALID);
    CHECK(k = f8_net_depth_to_space(net, src, 3, F8_ORDER_CRD));
    if (finish(net, k, "espcn")) return 1;

    net = f8_net_create();                                   /* edsr */
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 8, 6, 5, 8));
    CHECK(src = conv(net, x, 8, 64, 5, 8, 0, 0, 1));
    CHECK(k = f8_net_depth_to_space(net, src, 2, F8_ORDER_CRD));
    CHECK(k = conv(net, k, 16, 32, 6, 4, 0, 1, 0));
    if (finish(net, k, "edsr")) return 1;

    net = f8_net_create();                                   /* stem */
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 3, 16, 16, 8));
    CHECK(k = f8_net_space_to_depth(net, x, 4, F8_ORDER_DCR));
    CHECK(k = conv(net, k, 48, 32, 6, 8, 0, 0, 1));
    if (finish(net, k, "stem")) return 1;
    printf("ok\n");
    return 0;
}
