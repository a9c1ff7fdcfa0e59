"""TEST INFRASTRUCTURE ONLY: how every test of the compiled integration drivers (integration/*_main.cc) builds and starts them."""
import os
import subprocess

from conftest import ROOT

INTEG = os.path.join(ROOT, "integration")


def exe(name):
    return os.path.join(INTEG, "build", name)


def build():
    """The one `make -C integration`: every driver, under integration/build/."""
    r = subprocess.run(["make", "-C", INTEG], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def run(name, *args):
    """Run integration/build/<name> under a time limit of its own and return the finished process (stdout and stderr as text); a driver
    that does not end with status 0 fails the test with its stderr."""
    r = subprocess.run(["timeout", "-k", "10", "120", exe(name)] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, (name, r.returncode, r.stderr)
    return r
