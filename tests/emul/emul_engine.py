"""TEST-ONLY helper: an Engine bound to the CPU emulation build of the kernel sources (hip_emul.h)."""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_LIB = os.path.join(_HERE, "libscanfold_emul.so")


def build():
    subprocess.check_call(["make", "-C", _HERE, "-s"])


def emul_engine(paramset=None):
    from scanfold_amd._lib import Engine
    build()
    return Engine(device=0, paramset=paramset, lib_path=EMUL_LIB)


def launch_log(eng, clear=True):
    """The kernels the emulation build has launched since the log was last cleared, as their call sites spell them."""
    fn = eng.lib.sfemul_launch_log
    fn.restype = ctypes.c_char_p
    names = fn().decode().split("\n")[:-1]
    if clear:
        eng.lib.sfemul_launch_log_clear()
    return names
