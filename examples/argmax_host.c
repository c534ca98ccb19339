/* Channel argmax outputs through the C ABI, plain C99 against include/f8net.h (see examples/host_demo.c for the build line).
 *
 * Records the tail of a segmentation net — a 1x1 classifier to 21 classes on a 16 x 16 map, bilinear x4 back to 64 x 64, the class map as uint8 —,
 * finalizes it (planning needs no GPU), prints the plan and the output's kind and size, and destroys the handle.  The upsampled logits are read by
 * nothing else, so the plan holds one launch `upsample_bilinear+argmax_u8:` and no upsample launch: they never exist.  A second handle marks the
 * classifier's result both ways (logits and classes side by side) and shows the two-launch form.  Then it walks the refusals of f8_net_output_argmax.
 * The library's host code is built with AddressSanitizer and UndefinedBehaviorSanitizer and linked with this file into a stand-alone program
 * (DESIGN.md 4.5p).  It touches no device. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "f8net.h"

#define CHECK(x) do { int rc_ = (x); if (rc_ < 0) { fprintf(stderr, "%s failed: %s\n", #x, f8_last_error()); return 1; } } while (0)
#define EXPECT(x, code) do { int rc_ = (x); if (rc_ != (code)) { fprintf(stderr, "%s: status %d, expected %d\n", #x, rc_, (code)); return 1; } } while (0)

static int32_t wbuf[300 * 8];

static int conv1x1(f8_net* net, int src, int cin, int cout) {
    f8_conv_desc d;
    int i;
    memset(&d, 0, sizeof d);
    d.cin = cin; d.cout = cout; d.kernel = 1; d.stride = 1; d.pad = 0; d.groups = 1;
    d.weight_fl = 5; d.input_fl = 8; d.input_signed = 0; d.quant_input = 0; d.relu = 0;
    for (i = 0; i < cin * cout; ++i) wbuf[i] = (i * 7 + cout) % 11 - 5;
    return f8_net_conv(net, src, &d, wbuf, NULL);
}

static int print_plan(const f8_net* net, const char* title) {
    const size_t need = f8_net_describe(net, NULL, 0);
    char* plan = (char*)malloc(need);
    int k;
    if (!plan) return 1;
    f8_net_describe(net, plan, need);
    printf("== %s: %d launches\n%s", title, f8_net_num_launches(net), plan);
    free(plan);
    for (k = 0; k < f8_net_num_outputs(net); ++k) {
        int C, H, W, fl, as_float;
        CHECK(f8_net_output_info(net, k, &C, &H, &W, &fl, &as_float));
        printf("output %d: kind %d, %d x %d x %d, fraclen %d\n", k, f8_net_output_kind(net, k), C, H, W, fl);
    }
    printf("output 0: %lu elements an image\n", (unsigned long)f8_net_output_elems(net));
    return 0;
}

int main(void) {
    int x, cls, seg, one, wide, k;
    f8_net* net = f8_net_create();
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 8, 16, 16, 8));
    CHECK(cls = conv1x1(net, x, 8, 21));
    CHECK(seg = f8_net_upsample(net, cls, F8_UP_BILINEAR, 4, 4));
    CHECK(f8_net_set_label(net, seg, "seg"));
    CHECK(one = conv1x1(net, x, 8, 1));
    CHECK(wide = conv1x1(net, x, 8, 300));
    /* refusals */
    EXPECT(f8_net_output_argmax(NULL, seg, F8_IDX_U8), F8_ERR_INVALID);
    EXPECT(f8_net_output_argmax(net, 99, F8_IDX_U8), F8_ERR_INVALID);
    EXPECT(f8_net_output_argmax(net, -1, F8_IDX_U8), F8_ERR_INVALID);
    EXPECT(f8_net_output_argmax(net, seg, 2), F8_ERR_INVALID);
    EXPECT(f8_net_output_argmax(net, seg, 0), F8_ERR_INVALID);
    EXPECT(f8_net_output_argmax(net, one, F8_IDX_I32), F8_ERR_INVALID);        /* C < 2 */
    EXPECT(f8_net_output_argmax(net, wide, F8_IDX_U8), F8_ERR_UNSUPPORTED);    /* 300 classes do not fit uint8 */
    EXPECT(f8_net_output_kind(net, 0), F8_ERR_INVALID);                       /* no output yet */
    CHECK(k = f8_net_output_argmax(net, seg, F8_IDX_U8));
    if (k != 0) { fprintf(stderr, "first output has index %d\n", k); return 1; }
    EXPECT(f8_net_output_argmax(net, seg, F8_IDX_I32), F8_ERR_INVALID);        /* a second argmax mark on one tensor */
    EXPECT(f8_net_output_kind(net, 0), 2);
    CHECK(f8_net_finalize(net, 3));
    if (f8_net_output_elems(net) != 64u * 64u) { fprintf(stderr, "output 0 has %lu elements\n", (unsigned long)f8_net_output_elems(net)); return 1; }
    if (print_plan(net, "segmentation tail, fused")) return 1;
    EXPECT(f8_net_output_argmax(net, cls, F8_IDX_U8), F8_ERR_STATE);
    f8_net_destroy(net);

    /* logits and classes side by side: the tensor carries one mark of each kind; one output too many is refused */
    net = f8_net_create();
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 8, 16, 16, 8));
    CHECK(cls = conv1x1(net, x, 8, 21));
    CHECK(f8_net_output(net, cls, 0));
    CHECK(k = f8_net_output_argmax(net, cls, F8_IDX_I32));
    if (k != 1) { fprintf(stderr, "second output has index %d\n", k); return 1; }
    for (k = 2; k < F8_MAX_OUTPUTS; ++k) { int t; CHECK(t = conv1x1(net, x, 8, 4)); CHECK(f8_net_output_argmax(net, t, F8_IDX_U8)); }
    EXPECT(f8_net_output_argmax(net, x, F8_IDX_U8), F8_ERR_UNSUPPORTED);
    CHECK(f8_net_finalize(net, 2));
    EXPECT(f8_net_output_kind(net, 0), 0);
    EXPECT(f8_net_output_kind(net, 1), 3);
    EXPECT(f8_net_output_kind(net, F8_MAX_OUTPUTS), F8_ERR_INVALID);
    if (print_plan(net, "logits and classes")) return 1;
    f8_net_destroy(net);
    printf("ok\n");
    return 0;
}
