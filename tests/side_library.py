"""What the CPU tests of the five side libraries (include/agt_<name>.h -> libagt_<name>.so) check in the same way: the library builds and
exports exactly what its header declares and its Python module lists.  Each test keeps its own kernel list and resource thresholds."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def declared_symbols(name):
    text = open(os.path.join(ROOT, "include", "agt_%s.h" % name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(agt_[a-z0-9_]+)\s*\(", text)))


def built(module, name):
    """build(); libagt_<name>.so exists and exports declared_symbols(name) == module.SYMBOLS -> its kernels' resource rows"""
    import __graft_entry__ as g
    g.build()
    import kernel_resources
    assert os.path.exists(module.LIB_PATH), "make all does not build libagt_%s.so" % name
    out = subprocess.check_output(["nm", "-D", "--defined-only", module.LIB_PATH], text=True)
    exported = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    assert exported == set(declared_symbols(name)) == set(module.SYMBOLS)
    return kernel_resources.kernel_rows(module.LIB_PATH)
