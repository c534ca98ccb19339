"""examples/rect_host.c: f8_net_conv_rect from plain C99, compiled and run against expected values."""
from graph_cases import sanitized_host_program


def test_host_code_under_asan_and_ubsan():
    """The example records 1x1 -> 1x7 -> 7x1 and a SAME-padded 3x3 / 2 -> depthwise 1x11 -> depthwise 11x1 / 2 through the C ABI, walks the refusals,
    checks the output shapes and fraclens itself, compares a square geometry through the new call with f8_net_conv, finalizes, describes and destroys.
    f8_net.cpp's host side is compiled with AddressSanitizer and UndefinedBehaviorSanitizer and linked with the library's other objects into that
    stand-alone program."""
    out = sanitized_host_program('rect_host.c')
    assert out.rstrip().endswith('ok')
    assert '== 1x7 -> 7x1: 5 launches, output 64 x 17 x 17 at fraclen 13' in out
    assert out.count('conv1x7s1_t64x64x64:b_1x7') == 1 and out.count('conv7x1s1_t64x64x64:b_7x1') == 1
    assert '== same head + strips: 5 launches, output 32 x 8 x 8 at fraclen 13' in out
    assert out.count('conv3x3s2_t128x32x32:same_head') == 1 and out.count('dwconv1x11s1:strip_w') == 1 and out.count('dwconv11x1s2:strip_h') == 1
