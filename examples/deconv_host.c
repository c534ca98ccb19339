/* Transposed convolutions through the C ABI, plain C99 against include/f8net.h (see examples/host_demo.c for the build line).
 *
 * Records one U-Net step with f8_net_conv_transpose, finalizes it (planning needs no GPU), prints the plan and destroys the handle:
 *   skip = conv 3x3 of the input (32 channels, 16 x 16)          down = conv 3x3 / 2 of skip (64 channels, 8 x 8)
 *   mid  = conv 3x3 of down (64 channels)                        up   = deconv 2x2 / 2 of mid (32 channels, 16 x 16)
 *   out  = conv 3x3 of concat(up, skip) to 5 classes, output 0
 * The transposed conv plans deconv2x2s2: on f8::deconv_kernel<1>; the concat behind it runs in its byte-gather mode, so the transposed conv writes the
 * concat's int8 format itself.  A second handle records one transposed conv per phase shape of the packer — taps on every phase (4x4 / 2), phases
 * without a tap (1x1 / 2, 3x3 / 4), the largest kernel and stride (8x8 / 4 / pad 2 / output_padding 3) on 1 x 1, 1 x 3 and 3 x 5 maps — and stride 1,
 * which is recorded as a plain conv.  Then it walks the refusals.  The library's host code is built with AddressSanitizer and
 * UndefinedBehaviorSanitizer and linked with this file into a stand-alone program. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "f8net.h"

#define CHECK(x) do { int rc_ = (x); if (rc_ < 0) { fprintf(stderr, "%s failed: %s\n", #x, f8_last_error()); return 1; } } while (0)
#define EXPECT(x, code) do { int rc_ = (x); if (rc_ != (code)) { fprintf(stderr, "%s: status %d, expected %d\n", #x, rc_, (code)); return 1; } } while (0)

static int32_t wbuf[96 * 64 * 64];

static void desc(f8_conv_desc* d, int cin, int cout, int k, int stride, int pad, int w_fl, int in_fl, int quant, int relu) {
    memset(d, 0, sizeof *d);
    d->cin = cin; d->cout = cout; d->kernel = k; d->stride = stride; d->pad = pad; d->groups = 1;
    d->weight_fl = w_fl; d->input_fl = in_fl; d->input_signed = 0; d->quant_input = quant; d->relu = relu;
}

static void fill(int n, int salt) {
    int i;
    for (i = 0; i < n; ++i) wbuf[i] = (i * 7 + salt) % 11 - 5;
}

static int conv(f8_net* net, int src, int cin, int cout, int k, int stride, int w_fl, int in_fl, int quant, int relu) {
    f8_conv_desc d;
    desc(&d, cin, cout, k, stride, k / 2, w_fl, in_fl, quant, relu);
    fill(cin * cout * k * k, cout);
    return f8_net_conv(net, src, &d, wbuf, NULL);
}

static int deconv(f8_net* net, int src, int cin, int cout, int k, int stride, int pad, int op, int relu) {
    f8_conv_desc d;
    desc(&d, cin, cout, k, stride, pad, 6, 4, 1, relu);
    fill(cin * cout * k * k, cout + k);
    return f8_net_conv_transpose(net, src, &d, op, wbuf, NULL);
}

static int show(f8_net* net, const char* title) {
    int C, H, W, fl, as_float;
    size_t need;
    char* plan;
    CHECK(f8_net_output_info(net, 0, &C, &H, &W, &fl, &as_float));
    need = f8_net_describe(net, NULL, 0);
    plan = (char*)malloc(need);
    if (!plan) return 1;
    f8_net_describe(net, plan, need);
    printf("== %s: %d launches, output %d x %d x %d at fraclen %d\n%s", title, f8_net_num_launches(net), C, H, W, fl, plan);
    free(plan);
    return 0;
}

int main(void) {
    int x, skip, down, mid, up, cat, out, srcs[2], t, u, sum, C, H, W, fl, as_float, i;
    f8_conv_desc d;
    /* ---- the U-Net step */
    f8_net* net = f8_net_create();
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 8, 16, 16, 8));
    CHECK(skip = conv(net, x, 8, 32, 3, 1, 2, 8, 0, 1));            /* fraclen 10 */
    CHECK(down = conv(net, skip, 32, 64, 3, 2, 6, 4, 1, 1));
    CHECK(mid = conv(net, down, 64, 64, 3, 1, 6, 4, 1, 1));
    /* refusals */
    desc(&d, 64, 32, 2, 2, 0, 6, 4, 1, 1);
    fill(64 * 32 * 4, 1);
    EXPECT(f8_net_conv_transpose(NULL, mid, &d, 0, wbuf, NULL), F8_ERR_INVALID);
    EXPECT(f8_net_conv_transpose(net, mid, NULL, 0, wbuf, NULL), F8_ERR_INVALID);
    EXPECT(f8_net_conv_transpose(net, mid, &d, 0, NULL, NULL), F8_ERR_INVALID);
    EXPECT(f8_net_conv_transpose(net, 99, &d, 0, wbuf, NULL), F8_ERR_INVALID);
    EXPECT(f8_net_conv_transpose(net, mid, &d, -1, wbuf, NULL), F8_ERR_INVALID);
    EXPECT(f8_net_conv_transpose(net, mid, &d, 2, wbuf, NULL), F8_ERR_INVALID);
    d.cin = 32; EXPECT(f8_net_conv_transpose(net, mid, &d, 0, wbuf, NULL), F8_ERR_INVALID); d.cin = 64;
    wbuf[5] = 128; EXPECT(f8_net_conv_transpose(net, mid, &d, 0, wbuf, NULL), F8_ERR_INVALID); wbuf[5] = 1;
    d.kernel = 9; EXPECT(f8_net_conv_transpose(net, mid, &d, 0, wbuf, NULL), F8_ERR_UNSUPPORTED); d.kernel = 2;
    d.stride = 5; EXPECT(f8_net_conv_transpose(net, mid, &d, 0, wbuf, NULL), F8_ERR_UNSUPPORTED); d.stride = 2;
    d.pad = 2; EXPECT(f8_net_conv_transpose(net, mid, &d, 0, wbuf, NULL), F8_ERR_UNSUPPORTED); d.pad = 0;
    d.groups = 2; EXPECT(f8_net_conv_transpose(net, mid, &d, 0, wbuf, NULL), F8_ERR_UNSUPPORTED); d.groups = 1;
    /* the decoder */
    CHECK(up = deconv(net, mid, 64, 32, 2, 2, 0, 0, 1));            /* fraclen 10, the skip's */
    CHECK(f8_net_set_label(net, up, "up"));
    srcs[0] = up; srcs[1] = skip;
    CHECK(cat = f8_net_concat(net, srcs, 2));
    CHECK(f8_net_set_label(net, cat, "cat"));
    CHECK(out = conv(net, cat, 64, 5, 3, 1, 6, 4, 1, 0));
    CHECK(f8_net_output(net, out, 0));
    CHECK(f8_net_finalize(net, 3));
    CHECK(f8_net_output_info(net, 0, &C, &H, &W, &fl, &as_float));
    if (C != 5 || H != 16 || W != 16 || fl != 10) { fprintf(stderr, "output is %d x %d x %d at fraclen %d\n", C, H, W, fl); return 1; }
    if (show(net, "unet step")) return 1;
    EXPECT(f8_net_conv_transpose(net, mid, &d, 0, wbuf, NULL), F8_ERR_STATE);
    f8_net_destroy(net);

    /* ---- the packer's phase shapes, on three maps */
    for (i = 0; i < 3; ++i) {
        static const int hw[3][2] = {{1, 1}, {1, 3}, {3, 5}};
        net = f8_net_create();
        if (!net) return 1;
        CHECK(x = f8_net_input(net, 8, hw[i][0], hw[i][1], 8));
        CHECK(t = conv(net, x, 8, 40, 1, 1, 5, 8, 0, 1));
        CHECK(u = deconv(net, t, 40, 21, 4, 2, 1, 0, 0));
        CHECK(f8_net_output(net, u, 0));
        CHECK(u = deconv(net, t, 40, 21, 1, 2, 0, 1, 1));
        CHECK(f8_net_output(net, u, 0));
        CHECK(u = deconv(net, t, 40, 21, 3, 4, 1, 2, 0));
        CHECK(f8_net_output(net, u, 0));
        CHECK(u = deconv(net, t, 40, 96, 8, 4, 2, 3, 0));
        CHECK(f8_net_output(net, u, 0));
        CHECK(sum = deconv(net, t, 40, 21, 3, 1, 1, 0, 0));         /* stride 1: a plain conv */
        CHECK(f8_net_output(net, sum, 1));
        CHECK(f8_net_finalize(net, 2));
        if (show(net, "phase shapes")) return 1;
        f8_net_destroy(net);
    }
    printf("ok\n");
    return 0;
}
