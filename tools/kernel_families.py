"""tools/kernel_families.py -- which family a path kernel's row of a kernel trace or a listing belongs to, by its name and its template arguments.

The forms of k_shade and of the secondary-ray kernels that take the tables of fh_set_env_sampling / fh_set_light_sampling are instantiations of the plain kernel's
template with the tables as trailing template arguments (render.hip): k_shade<68u, 2, fh::EnvTable>, k_shade<64u, 2, fh::UnreadEnvTable, fh::LightTable>,
k_trace_secondary_stream<false, true, false, float const*>.  The benchmarks' records keep the names these forms had as kernels of their own -- k_shade_env, k_shade_lt,
k_trace_secondary_stream_lt ... -- so that new records compare with the committed ones.  k_tail_env and k_tail_lt are still kernels of that name."""
import functools
import re
import subprocess

PATH_KERNELS = ("k_shade", "k_tail", "k_trace_secondary_static", "k_trace_secondary_coop", "k_trace_secondary_stream", "k_trace_merged_stream")
_PAT = re.compile(r"\b(" + "|".join(PATH_KERNELS) + r")(_env|_lt)?<")


@functools.lru_cache(maxsize=None)
def template_id(name):
    """(family by name, 'kernel<arguments>') of a path kernel's demangled or mangled name; (None, None) for any other"""
    if name.startswith("_Z"):
        name = subprocess.run(["c++filt", name.split(".")[0]], capture_output=True, text=True).stdout.strip()
    m = _PAT.search(name)
    if not m:
        return None, None
    i, depth = m.end(), 1
    while i < len(name) and depth:
        depth += {"<": 1, ">": -1}.get(name[i], 0)
        i += 1
    return m.group(1) + (m.group(2) or ""), name[m.start():i]


def family(name):
    """k_shade, k_shade_env or k_shade_lt (and so on); None for a kernel that is no path kernel"""
    kernel, tid = template_id(name)
    if kernel is None or kernel.endswith(("_env", "_lt")):
        return kernel
    if "LightTable" in tid or "float const*" in tid:
        return kernel + "_lt"
    if re.search(r"\bEnvTable\b", tid):  # (not UnreadEnvTable)
        return kernel + "_env"
    return kernel
