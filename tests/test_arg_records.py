"""The two argument records of f8_internal.h (Requant, FastDiv) and the one fast-instance rule, checked by a stand-alone program: no GPU, nothing
loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fast_divisor_requant_of_and_the_u8_rule_under_asan_and_ubsan(tmp_path):
    """tests/arg_records_check.cpp, host side under AddressSanitizer + UndefinedBehaviorSanitizer: fast_divisor(d) by the documented formula equals
    n / d for 19 divisors x (8 edge dividends, k d - 1 and k d for 64 seeded k, 10^5 seeded random values); Requant::of gives (-127, 127, 0) /
    (0, 255, 0x80808080); u8_shr() holds exactly for unsigned formats with 1 <= n <= 30 over n in -31 .. 31 and both signs, u8_float() adds n <= 16."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    assert os.path.exists(hipcc)
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    obj, exe = str(tmp_path / 'arg_records_check.o'), str(tmp_path / 'arg_records_check')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O1', '-g', '-std=c++17', '-Wall', '-Werror'] + [a for s in san for a in ('-Xarch_host', s)] +
                          ['-x', 'hip', '-c', os.path.join(ROOT, 'tests', 'arg_records_check.cpp'), '-o', obj])
    subprocess.check_call([hipcc, '--offload-arch=gfx950'] + san + [obj, '-o', exe])
    env = dict(os.environ, LD_LIBRARY_PATH='/opt/rocm/lib:' + os.environ.get('LD_LIBRARY_PATH', ''), ASAN_OPTIONS='detect_leaks=1')
    r = subprocess.run([exe], text=True, capture_output=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr
    assert r.stdout.rstrip().endswith('ok') and '1902584 divisions checked, 0 bad' in r.stdout, r.stdout
