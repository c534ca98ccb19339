/* The 256-entry table op through the C ABI, plain C99 against include/f8net.h (see examples/host_demo.c for the build line; link with -lm).
 *
 * Records three graphs with f8_net_table, finalizes each (planning needs no GPU: the byte tables are composed on the host there), prints the plans
 * and destroys the handles:
 *   se       a squeeze-and-excitation block with a TRUE sigmoid gate: 1x1 to 48, global pool, two FCs, sigmoid table, channel gate, 1x1
 *            -> one table+chmul_i8: launch (the table emits none)
 *   extreme  a signed table holding INT32_MIN, INT32_MAX and 0, read in two int8 formats by a right and by a left shift  -> table_i8:
 *   output   the same table as a network output and read in three formats                                                -> table_i32: and requant:
 * and walks the refusals of the entry point.  tests/test_table_plan.py builds the library's host code with AddressSanitizer and
 * UndefinedBehaviorSanitizer and runs this program against it. */
#include <math.h>
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

static int fc(f8_net* net, int src, int cin, int cout, int w_fl, int in_fl, int sgn) {
    f8_linear_desc d;
    int i;
    memset(&d, 0, sizeof d);
    d.in_features = cin; d.out_features = cout; d.weight_fl = w_fl; d.input_fl = in_fl; d.input_signed = sgn; d.quant_input = 1;
    for (i = 0; i < cin * cout; ++i) wbuf[i] = (i * 5 + cin) % 13 - 6;
    return f8_net_linear(net, src, &d, wbuf, NULL);
}

static f8_table_desc fmt(int in_fl, int in_signed, int out_fl) {
    f8_table_desc d;
    d.in_fl = in_fl; d.in_signed = in_signed; d.out_fl = out_fl;
    return d;
}

/* sigmoid on the grid of a signed index format: entry i is q = i - 128 */
static void sigmoid_table(int32_t t[256], int in_fl, int out_fl) {
    int i;
    for (i = 0; i < 256; ++i) t[i] = (int32_t)nearbyint(ldexp(1.0 / (1.0 + exp(-ldexp((double)(i - 128), -in_fl))), out_fl));
}

static int finish(f8_net* net, const char* what) {
    size_t need;
    char* plan;
    int32_t t[256] = {0};
    f8_table_desc d = fmt(4, 0, 4);
    CHECK(f8_net_finalize(net, 3));
    need = f8_net_describe(net, NULL, 0);
    plan = (char*)malloc(need);
    if (!plan) return 1;
    f8_net_describe(net, plan, need);
    printf("== %s: %d launches\n%s", what, f8_net_num_launches(net), plan);
    free(plan);
    EXPECT(f8_net_table(net, 1, &d, t), F8_ERR_STATE);
    f8_net_destroy(net);
    return 0;
}

int main(void) {
    int x, src, pool, f1, f2, gate, m, k, t, i, far;
    int32_t sig[256], ext[256];
    f8_table_desc d;
    f8_mul_desc md;
    f8_net* net;

    sigmoid_table(sig, 4, 12);
    for (i = 0; i < 256; ++i) ext[i] = i % 5 == 0 ? INT32_MIN : i % 5 == 1 ? INT32_MAX : i % 5 == 2 ? 0 : (int32_t)((uint32_t)i * 2654435761u);

    net = f8_net_create();                                   /* se */
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 8, 7, 7, 8));
    CHECK(src = conv(net, x, 8, 48, 5, 8, 0, 0, 1));                     /* fraclen 13 */
    CHECK(pool = f8_net_avgpool_sum(net, src, 6));                       /* 19 */
    CHECK(f1 = fc(net, pool, 48, 16, 5, 4, 0));                          /* 9 */
    CHECK(f2 = fc(net, f1, 16, 48, 6, 3, 1));                            /* 9 */
    d = fmt(4, 1, 12);
    EXPECT(f8_net_table(net, f2, NULL, sig), F8_ERR_INVALID);
    EXPECT(f8_net_table(net, f2, &d, NULL), F8_ERR_INVALID);
    EXPECT(f8_net_table(net, 99, &d, sig), F8_ERR_INVALID);
    EXPECT(f8_net_table(net, -1, &d, sig), F8_ERR_INVALID);
    d = fmt(9, 0, 12);
    EXPECT(f8_net_table(net, f2, &d, sig), F8_ERR_INVALID);              /* unsigned fraclen above 8 */
    d = fmt(8, 1, 12);
    EXPECT(f8_net_table(net, f2, &d, sig), F8_ERR_INVALID);              /* signed fraclen above 7 */
    d = fmt(-1, 0, 12);
    EXPECT(f8_net_table(net, f2, &d, sig), F8_ERR_INVALID);
    d = fmt(4, 1, 39);
    EXPECT(f8_net_table(net, f2, &d, sig), F8_ERR_INVALID);              /* no 8-bit format reads fraclen 39 */
    d = fmt(4, 1, -1);
    EXPECT(f8_net_table(net, f2, &d, sig), F8_ERR_INVALID);
    CHECK(far = fc(net, pool, 48, 16, 31, 8, 0));                        /* fraclen 39 */
    d = fmt(8, 0, 12);
    EXPECT(f8_net_table(net, far, &d, sig), F8_ERR_INVALID);             /* shift 31 */
    d = fmt(4, 1, 12);
    CHECK(gate = f8_net_table(net, f2, &d, sig));
    sig[5] = 77;                                                         /* the op copied the table at the call */
    md.a_fl = 4; md.a_signed = 0; md.b_fl = 8; md.b_signed = 0; md.relu = 0;
    CHECK(m = f8_net_mul(net, src, gate, &md));
    CHECK(k = conv(net, m, 48, 32, 6, 2, 0, 1, 0));
    CHECK(f8_net_output(net, k, 0));
    if (finish(net, "se")) return 1;

    net = f8_net_create();                                   /* extreme */
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 8, 9, 11, 8));
    CHECK(src = conv(net, x, 8, 20, 5, 8, 0, 0, 0));
    d = fmt(6, 1, 30);
    CHECK(t = f8_net_table(net, src, &d, ext));
    CHECK(k = conv(net, t, 20, 32, 6, 6, 1, 1, 0));                      /* a right shift by 24 */
    CHECK(f8_net_output(net, k, 0));
    d = fmt(6, 1, 0);
    CHECK(t = f8_net_table(net, src, &d, ext));
    CHECK(k = conv(net, t, 20, 32, 6, 8, 0, 1, 0));                      /* a left shift by 8 */
    CHECK(f8_net_output(net, k, 0));
    if (finish(net, "extreme")) return 1;

    net = f8_net_create();                                   /* output */
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 8, 7, 7, 8));
    CHECK(src = conv(net, x, 8, 64, 5, 8, 0, 0, 1));
    d = fmt(8, 0, 36);
    CHECK(t = f8_net_table(net, src, &d, ext));
    CHECK(f8_net_output(net, t, 0));
    for (i = 0; i < 3; ++i) {
        CHECK(k = conv(net, t, 64, 32, 6, 8 - i, i & 1, 1, 0));          /* shifts 28, 29, 30: three formats */
        CHECK(f8_net_output(net, k, 0));
    }
    if (finish(net, "output")) return 1;
    printf("ok\n");
    return 0;
}
