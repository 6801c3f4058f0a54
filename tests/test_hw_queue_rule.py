"""GPU_MAX_HW_QUEUES at load time (csrc/eh_host_queues.h, eh_runtime_defaults in csrc/eh_engine.hip): the library asks for eight
hardware queues when the variable is not set or holds a plain decimal number below eight, and leaves every other value alone.
First the rule by itself, a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/hipemu/hw_queue_rule.cpp); then the built library, loaded into fresh processes.  No GPU: loading makes no HIP call."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
LIB = os.path.join(ROOT, "erlamsa_amd", "liberlamsa_hip.so")

UNSET = "-"                                     # hw_queue_rule's argument for "the variable is not set"
WRITE_8 = [UNSET, "0", "1", "4", "7"]
LEAVE = ["", "8", "9", "32", "64", " 4", "4 ", "+4", "-1", "4x", "0x4", "1234567890" * 4]


def test_rule_alone_under_sanitizers():
    """not set and the plain decimals below eight -> write 8; "", 8 and more (a 40-digit number too), blanks, signs, trailing
    text and a hexadecimal prefix -> leave: one line per value, no sanitizer report"""
    import build_hw_queue_rule
    exe = build_hw_queue_rule.build()
    values = WRITE_8 + LEAVE
    r = subprocess.run([exe] + values, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    want = ["%s -> write 8" % v for v in WRITE_8] + ["%s -> leave" % v for v in LEAVE] + ["hw_queue_rule ok", ""]
    assert lines == want
    assert r.stderr == ""


# the child: load the library, then ask libc - os.environ is a snapshot taken when the interpreter started
CHILD = ("import ctypes, sys\n"
         "ctypes.CDLL(sys.argv[1])\n"
         "libc = ctypes.CDLL(None)\n"
         "libc.getenv.restype = ctypes.c_char_p\n"
         "v = libc.getenv(b'GPU_MAX_HW_QUEUES')\n"
         "sys.stdout.write('unset' if v is None else 'value:' + v.decode())\n")


@pytest.mark.skipif(not os.path.exists(LIB), reason="liberlamsa_hip.so is not built")
@pytest.mark.parametrize("preset,after", [(None, "8"), ("4", "8"), ("8", "8"), ("16", "16"), ("abc", "abc")])
def test_variable_after_the_library_is_loaded(preset, after):
    """a fresh process with the variable not set / 4 / 8 / 16 / abc loads the built library: getenv then gives 8 / 8 / 8 / 16 / abc"""
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    if preset is not None:
        env["GPU_MAX_HW_QUEUES"] = preset
    r = subprocess.run([sys.executable, "-c", CHILD, LIB], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout == "value:" + after
