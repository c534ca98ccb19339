/* Rectangular convolutions through the C ABI, plain C99 against include/f8net.h (see examples/host_demo.c for the build line).
 *
 * Records, finalizes (planning needs no GPU), prints the plan of and destroys two handles:
 *   an Inception-style pair   in (64 channels, 17 x 17) -> conv 1x1 -> conv 1x7, pads (0, 3, 0, 3) -> conv 7x1, pads (3, 0, 3, 0), output
 *   a TF-style head           in (3 channels, 32 x 32) -> conv 3x3 / 2 with SAME pads (0, 0, 1, 1) -> depthwise 1x11 -> depthwise 11x1 / 2, output
 * f8_net_conv_rect takes the f8_conv_desc of f8_net_conv with kernel = stride = pad = 0 and the geometry in an f8_conv_geom.  The plain convs plan
 * conv1x7s1_t...: and conv7x1s1_t...: on f8::conv_igemm_kernel, the strips dwconv1x11s1: on f8::dwstrip_dot4_kernel<4> and dwconv11x1s2: on
 * f8::dwconvk_kernel.  A square, symmetric geometry through the same call records the node f8_net_conv records: the two plans are compared.  Then it
 * walks the refusals.  The library's host code is built with AddressSanitizer and UndefinedBehaviorSanitizer and linked with this file into a
 * stand-alone program. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "f8net.h"

#define CHECK(x) do { int rc_ = (x); if (rc_ < 0) { fprintf(stderr, "%s failed: %s\n", #x, f8_last_error()); return 1; } } while (0)
#define EXPECT(x, code) do { int rc_ = (x); if (rc_ != (code)) { fprintf(stderr, "%s: status %d, expected %d\n", #x, rc_, (code)); return 1; } } while (0)

static int32_t wbuf[64 * 64 * 31];

static void desc(f8_conv_desc* d, int cin, int cout, int groups, int w_fl, int in_fl, int quant, int relu) {
    memset(d, 0, sizeof *d);                                        /* kernel = stride = pad = 0: the geometry comes from the f8_conv_geom */
    d->cin = cin; d->cout = cout; d->groups = groups;
    d->weight_fl = w_fl; d->input_fl = in_fl; d->input_signed = 0; d->quant_input = quant; d->relu = relu;
}

static void geom(f8_conv_geom* g, int kh, int kw, int sh, int sw, int top, int left, int bottom, int right) {
    g->kh = kh; g->kw = kw; g->stride_h = sh; g->stride_w = sw;
    g->pad_top = top; g->pad_left = left; g->pad_bottom = bottom; g->pad_right = right; g->dilation = 1;
}

static void fill(int n, int salt) {
    int i;
    for (i = 0; i < n; ++i) wbuf[i] = (i * 7 + salt) % 11 - 5;
}

static int rect(f8_net* net, int src, const f8_conv_desc* d, const f8_conv_geom* g) {
    fill(d->cout * (d->cin / d->groups) * g->kh * g->kw, d->cout + g->kw);
    return f8_net_conv_rect(net, src, d, g, wbuf, NULL);
}

static char* plan_of(f8_net* net) {
    size_t need = f8_net_describe(net, NULL, 0);
    char* plan = (char*)malloc(need);
    if (plan) f8_net_describe(net, plan, need);
    return plan;
}

static int show(f8_net* net, const char* title, int wantC, int wantH, int wantW, int want_fl) {
    int C, H, W, fl, as_float;
    char* plan;
    CHECK(f8_net_output_info(net, 0, &C, &H, &W, &fl, &as_float));
    if (C != wantC || H != wantH || W != wantW || fl != want_fl) {
        fprintf(stderr, "%s: output is %d x %d x %d at fraclen %d, expected %d x %d x %d at %d\n", title, C, H, W, fl, wantC, wantH, wantW, want_fl);
        return 1;
    }
    plan = plan_of(net);
    if (!plan) return 1;
    printf("== %s: %d launches, output %d x %d x %d at fraclen %d\n%s", title, f8_net_num_launches(net), C, H, W, fl, plan);
    free(plan);
    return 0;
}

int main(void) {
    int x, t, pass;
    f8_conv_desc d;
    f8_conv_geom g;
    char* plans[2] = {NULL, NULL};
    f8_net* net;

    /* ---- 1x1 -> 1x7 -> 7x1 */
    net = f8_net_create();
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 64, 17, 17, 8));
    desc(&d, 64, 64, 1, 5, 8, 0, 1);
    geom(&g, 1, 1, 1, 1, 0, 0, 0, 0);
    CHECK(t = rect(net, x, &d, &g));                                /* fraclen 13 */
    desc(&d, 64, 64, 1, 9, 4, 1, 1);
    /* refusals */
    geom(&g, 1, 7, 1, 1, 0, 3, 0, 3);
    EXPECT(f8_net_conv_rect(NULL, t, &d, &g, wbuf, NULL), F8_ERR_INVALID);
    EXPECT(f8_net_conv_rect(net, t, NULL, &g, wbuf, NULL), F8_ERR_INVALID);
    EXPECT(f8_net_conv_rect(net, t, &d, NULL, wbuf, NULL), F8_ERR_INVALID);
    EXPECT(f8_net_conv_rect(net, t, &d, &g, NULL, NULL), F8_ERR_INVALID);
    EXPECT(f8_net_conv_rect(net, 99, &d, &g, wbuf, NULL), F8_ERR_INVALID);
    d.kernel = 7; EXPECT(f8_net_conv_rect(net, t, &d, &g, wbuf, NULL), F8_ERR_INVALID); d.kernel = 0;
    d.stride = 1; EXPECT(f8_net_conv_rect(net, t, &d, &g, wbuf, NULL), F8_ERR_INVALID); d.stride = 0;
    d.pad = 3; EXPECT(f8_net_conv_rect(net, t, &d, &g, wbuf, NULL), F8_ERR_INVALID); d.pad = 0;
    g.kw = 32; EXPECT(f8_net_conv_rect(net, t, &d, &g, wbuf, NULL), F8_ERR_INVALID); g.kw = 7;
    g.stride_w = 0; EXPECT(f8_net_conv_rect(net, t, &d, &g, wbuf, NULL), F8_ERR_INVALID); g.stride_w = 1;
    g.pad_left = 7; EXPECT(f8_net_conv_rect(net, t, &d, &g, wbuf, NULL), F8_ERR_INVALID); g.pad_left = 3;
    g.pad_top = 1; EXPECT(f8_net_conv_rect(net, t, &d, &g, wbuf, NULL), F8_ERR_INVALID); g.pad_top = 0;      /* a 1-wide axis takes no pad */
    g.dilation = 0; EXPECT(f8_net_conv_rect(net, t, &d, &g, wbuf, NULL), F8_ERR_INVALID); g.dilation = 1;
    d.groups = 4; EXPECT(f8_net_conv_rect(net, t, &d, &g, wbuf, NULL), F8_ERR_UNSUPPORTED); d.groups = 1;      /* grouped rectangles */
    d.groups = 64; g.kh = 3; g.pad_top = 1;                         /* a depthwise 3x7 is no strip */
    EXPECT(f8_net_conv_rect(net, t, &d, &g, wbuf, NULL), F8_ERR_UNSUPPORTED);
    d.groups = 1; g.kh = 1; g.pad_top = 0;
    /* the pair */
    CHECK(t = rect(net, t, &d, &g));
    CHECK(f8_net_set_label(net, t, "b_1x7"));
    geom(&g, 7, 1, 1, 1, 3, 0, 3, 0);
    CHECK(t = rect(net, t, &d, &g));
    CHECK(f8_net_set_label(net, t, "b_7x1"));
    CHECK(f8_net_output(net, t, 0));
    CHECK(f8_net_finalize(net, 3));
    if (show(net, "1x7 -> 7x1", 64, 17, 17, 13)) return 1;
    EXPECT(f8_net_conv_rect(net, t, &d, &g, wbuf, NULL), F8_ERR_STATE);
    f8_net_destroy(net);

    /* ---- SAME-padded 3x3 / 2 -> depthwise 1x11 -> depthwise 11x1 / 2 */
    net = f8_net_create();
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 3, 32, 32, 8));
    desc(&d, 3, 32, 1, 5, 8, 0, 1);
    geom(&g, 3, 3, 2, 2, 0, 0, 1, 1);
    CHECK(t = rect(net, x, &d, &g));                                /* (32 + 1 - 3) / 2 + 1 = 16 */
    CHECK(f8_net_set_label(net, t, "same_head"));
    desc(&d, 32, 32, 32, 9, 4, 1, 1);
    geom(&g, 1, 11, 1, 1, 0, 5, 0, 5);
    CHECK(t = rect(net, t, &d, &g));
    CHECK(f8_net_set_label(net, t, "strip_w"));
    geom(&g, 11, 1, 2, 2, 5, 0, 5, 0);
    CHECK(t = rect(net, t, &d, &g));                                /* stride 2 on both axes: 8 x 8 */
    CHECK(f8_net_set_label(net, t, "strip_h"));
    CHECK(f8_net_output(net, t, 0));
    CHECK(f8_net_finalize(net, 3));
    if (show(net, "same head + strips", 32, 8, 8, 13)) return 1;
    f8_net_destroy(net);

    /* ---- square + symmetric through f8_net_conv_rect is f8_net_conv */
    for (pass = 0; pass < 2; ++pass) {
        net = f8_net_create();
        if (!net) return 1;
        CHECK(x = f8_net_input(net, 32, 12, 12, 8));
        desc(&d, 32, 32, 1, 5, 8, 0, 1);
        fill(32 * 32 * 9, 3);
        if (pass) {
            geom(&g, 3, 3, 1, 1, 1, 1, 1, 1);
            CHECK(t = f8_net_conv_rect(net, x, &d, &g, wbuf, NULL));
        } else {
            d.kernel = 3; d.stride = 1; d.pad = 1;
            CHECK(t = f8_net_conv(net, x, &d, wbuf, NULL));
        }
        CHECK(f8_net_output(net, t, 0));
        CHECK(f8_net_finalize(net, 2));
        plans[pass] = plan_of(net);
        f8_net_destroy(net);
        if (!plans[pass]) return 1;
    }
    if (strcmp(plans[0], plans[1])) { fprintf(stderr, "square through f8_net_conv_rect plans differently:\n%s%s", plans[0], plans[1]); return 1; }
    free(plans[0]);
    free(plans[1]);
    printf("ok\n");
    return 0;
}
