/* Fixed-point multiply and hard gate through the C ABI, plain C99 against include/f8net.h (see examples/host_demo.c for the build line).
 *
 * Records three graphs with f8_net_mul / f8_net_hard_gate, finalizes each (planning needs no GPU), prints the plans and destroys the handles:
 *   se       a squeeze-and-excitation block with a hard-sigmoid gate: 1x1 to 48, global pool, two FCs, hard gate, channel gate, 1x1
 *            -> one hgate+chmul_i8: launch (the gate emits none)
 *   hswish   hard-swish of a conv result that is also a network output        -> hgate+mul_i32:
 *   shared   a hard gate read by the channel gate AND by a conv: not fusable  -> hgate: then chmul_i8:
 * and walks the refusals of both entry points.  tests/test_mul_plan.py builds the library's host code with AddressSanitizer and
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

static int fc(f8_net* net, int src, int cin, int cout, int w_fl, int in_fl, int sgn) {
    f8_linear_desc d;
    int i;
    memset(&d, 0, sizeof d);
    d.in_features = cin; d.out_features = cout; d.weight_fl = w_fl; d.input_fl = in_fl; d.input_signed = sgn; d.quant_input = 1;
    for (i = 0; i < cin * cout; ++i) wbuf[i] = (i * 5 + cin) % 13 - 6;
    return f8_net_linear(net, src, &d, wbuf, NULL);
}

static f8_mul_desc fmt(int a_fl, int a_signed, int b_fl, int b_signed, int relu) {
    f8_mul_desc d;
    d.a_fl = a_fl; d.a_signed = a_signed; d.b_fl = b_fl; d.b_signed = b_signed; d.relu = relu;
    return d;
}

static int finish(f8_net* net, const char* what) {
    size_t need;
    char* plan;
    f8_mul_desc d = fmt(4, 0, 4, 0, 0);
    CHECK(f8_net_finalize(net, 3));
    need = f8_net_describe(net, NULL, 0);
    plan = (char*)malloc(need);
    if (!plan) return 1;
    f8_net_describe(net, plan, need);
    printf("== %s: %d launches\n%s", what, f8_net_num_launches(net), plan);
    free(plan);
    EXPECT(f8_net_mul(net, 1, 1, &d), F8_ERR_STATE);
    EXPECT(f8_net_hard_gate(net, 1), F8_ERR_STATE);
    f8_net_destroy(net);
    return 0;
}

int main(void) {
    int x, src, other, pool, f1, f2, gate, m, k, deep;
    f8_mul_desc d;
    f8_net* net;

    net = f8_net_create();                                   /* se */
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 8, 7, 7, 8));
    CHECK(src = conv(net, x, 8, 48, 5, 8, 0, 0, 1));                     /* fraclen 13 */
    CHECK(other = conv(net, x, 8, 24, 5, 8, 0, 0, 1));
    CHECK(pool = f8_net_avgpool_sum(net, src, 6));                       /* 19 */
    CHECK(f1 = fc(net, pool, 48, 16, 5, 4, 0));                          /* 9 */
    CHECK(f2 = fc(net, f1, 16, 48, 6, 3, 1));                            /* 9 */
    CHECK(gate = f8_net_hard_gate(net, f2));
    d = fmt(4, 0, 5, 0, 0);
    EXPECT(f8_net_mul(net, src, gate, NULL), F8_ERR_INVALID);
    EXPECT(f8_net_mul(net, 99, gate, &d), F8_ERR_INVALID);
    EXPECT(f8_net_mul(net, src, -1, &d), F8_ERR_INVALID);
    EXPECT(f8_net_mul(net, src, other, &d), F8_ERR_INVALID);             /* 24 channels against 48 */
    EXPECT(f8_net_mul(net, gate, src, &d), F8_ERR_INVALID);              /* the vector is operand b, not a */
    d = fmt(9, 0, 5, 0, 0);
    EXPECT(f8_net_mul(net, src, gate, &d), F8_ERR_INVALID);              /* unsigned fraclen above 8 */
    d = fmt(4, 0, 8, 1, 0);
    EXPECT(f8_net_mul(net, src, gate, &d), F8_ERR_INVALID);              /* signed fraclen above 7 */
    d = fmt(4, 0, -1, 0, 0);
    EXPECT(f8_net_mul(net, src, gate, &d), F8_ERR_INVALID);
    EXPECT(f8_net_hard_gate(net, 99), F8_ERR_INVALID);
    CHECK(deep = fc(net, pool, 48, 16, 31, 0, 0));                       /* fraclen 31 */
    EXPECT(f8_net_hard_gate(net, deep), F8_ERR_INVALID);                 /* 6 * 2^31 does not fit */
    d = fmt(4, 0, 5, 0, 0);
    CHECK(m = f8_net_mul(net, src, gate, &d));
    CHECK(k = conv(net, m, 48, 32, 6, 2, 0, 1, 0));
    CHECK(f8_net_output(net, k, 0));
    if (finish(net, "se")) return 1;

    net = f8_net_create();                                   /* hswish */
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 8, 9, 11, 8));
    CHECK(src = conv(net, x, 8, 20, 5, 8, 0, 0, 0));
    CHECK(gate = f8_net_hard_gate(net, src));
    d = fmt(4, 1, 5, 0, 0);
    CHECK(m = f8_net_mul(net, src, gate, &d));
    CHECK(f8_net_output(net, m, 0));
    if (finish(net, "hswish")) return 1;

    net = f8_net_create();                                   /* shared */
    if (!net) return 1;
    CHECK(x = f8_net_input(net, 8, 7, 7, 8));
    CHECK(src = conv(net, x, 8, 64, 5, 8, 0, 0, 1));
    CHECK(pool = f8_net_avgpool_sum(net, src, 6));
    CHECK(f2 = fc(net, pool, 64, 64, 0, 4, 0));                          /* fraclen 4 */
    CHECK(gate = f8_net_hard_gate(net, f2));
    d = fmt(4, 0, 4, 0, 1);
    CHECK(m = f8_net_mul(net, src, gate, &d));
    CHECK(k = conv(net, m, 64, 32, 6, 2, 0, 1, 0));
    CHECK(f8_net_output(net, k, 0));
    CHECK(k = conv(net, gate, 64, 32, 6, 4, 0, 1, 0));
    CHECK(f8_net_output(net, k, 0));
    if (finish(net, "shared")) return 1;
    printf("ok\n");
    return 0;
}
