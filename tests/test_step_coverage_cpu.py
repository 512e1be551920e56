"""CPU tier: a ledger over the sources, read as text, that keeps every kernel reachable alone.
(i) Every launch_* function declared in a launch_*.h is called in an engine*_steps.cpp unit -- a step of apsu_he_debug_run_step -- or
stands in HOOKS below with the debug hook or public call that runs it alone.  (ii) Every __global__ kernel of kernels_*.hip and
mac_core.h is named in a hipLaunchKernelGGL of some launcher.  A new launcher without a step, or a kernel nobody launches, fails here.
Matched are launcher and kernel names only."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "apsu_amd", "csrc")

# launcher -> the Engine method that runs it alone on caller-given input (include/apsu_he.h: apsu_he_debug_*, apsu_he_query_values)
HOOKS = {
    "launch_cuckoo_locations": "debug_item_locations",
    "launch_cuckoo_insert": "debug_cuckoo_insert",
    "launch_query_values": "query_values",
    "launch_bucket_sort": "debug_bucket_locs",
}


def read(path):
    with open(path) as f:
        return f.read()


def code(text):
    """the text without its comments"""
    return re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)


def declared_launchers(header_text):
    """the launch_* names a header declares or defines: a name directly behind a return type, at the start of a line"""
    return set(re.findall(r"^(?:static |inline |template <[^>]*> )*(?:const )?[\w:]+[ \*&]+(launch_\w+)\(", code(header_text), flags=re.M))


def launchers():
    out = {}
    for h in sorted(glob.glob(os.path.join(SRC, "launch_*.h"))):
        for name in declared_launchers(read(h)):
            out[name] = os.path.basename(h)
    return out


def step_units():
    return sorted(glob.glob(os.path.join(SRC, "engine*_steps.cpp")))


def called_in_steps():
    return set(re.findall(r"\b(launch_\w+)\s*\(", "\n".join(code(read(p)) for p in step_units())))


def test_every_launcher_has_a_step_or_a_named_hook():
    decl, called = launchers(), called_in_steps()
    assert len(decl) > 60 and len(step_units()) >= 7, (len(decl), step_units())
    missing = sorted(n for n in decl if n not in called and n not in HOOKS)
    assert not missing, "launchers that neither a step of engine*_steps.cpp nor a hook of HOOKS runs alone: %s" % ", ".join("%s (%s)" % (n, decl[n]) for n in missing)


def test_the_hook_table_is_short_and_true():
    decl, called = launchers(), called_in_steps()
    engine_h = code(read(os.path.join(SRC, "engine.h")))
    units = "\n".join(code(read(p)) for p in glob.glob(os.path.join(SRC, "engine*.cpp")))
    for launcher, hook in HOOKS.items():
        assert launcher in decl, launcher                     # the launcher exists ...
        assert launcher not in called, launcher               # ... has no step (else it leaves the table) ...
        assert re.search(r"\b%s\s*\(" % hook, engine_h), hook   # ... the hook is an Engine method ...
        assert re.search(r"\b%s\s*\(" % launcher, units), launcher      # ... and the engine calls the launcher


def test_the_ledger_sees_a_launcher_without_a_step():
    """the check on a header of its own making: one declaration more is one name more, and it is reported"""
    extra = "// a comment that names launch_in_a_comment(\nvoid launch_made_up(const u64 *in, u64 *out, hipStream_t st);\nconst u64 *launch_made_up_too(int x);\n"
    assert declared_launchers(extra) == {"launch_made_up", "launch_made_up_too"}
    assert "launch_made_up" not in called_in_steps() and "launch_made_up" not in HOOKS


def test_every_kernel_is_launched_by_a_launcher():
    files = sorted(glob.glob(os.path.join(SRC, "kernels_*.hip"))) + [os.path.join(SRC, "mac_core.h")]
    text = "\n".join(code(read(p)) for p in files)
    head = r"__global__[ \t]+(?:__launch_bounds__[ \t]*\([^;{\n]*?\)[ \t]*)?void"
    kernels = set(re.findall(head + r"\s+(\w+)\s*\(", text))
    # a kernel's head behind a macro (mac_core.h: MAC_LANE_FN, which the CPU tier defines as a plain function): the names defined with it
    macros = re.findall(r"^#define[ \t]+(\w+)[ \t]+" + head + r"[ \t]*$", text, flags=re.M)
    for m in macros:
        kernels |= set(re.findall(r"^%s[ \t]+(\w+)\s*\(" % m, text, flags=re.M))
    assert len(re.findall(r"__global__", text)) == len(re.findall(head + r"\s+\w+\s*\(", text)) + len(macros)      # no head of another shape
    launched = set(re.findall(r"hipLaunchKernelGGL\(\s*\(*\s*(\w+)", text))
    # the transforms launch an instance picked from a table of forms, form_kernel(<kernel>_forms, ..): the table's name carries the kernel's,
    # and its rows name the kernel's instances
    for table in re.findall(r"hipLaunchKernelGGL\(\s*form_kernel\(\s*(\w+)_forms\b", text):
        if re.search(r"\b%s_forms\[\]" % table, text) and re.search(r"\b%s<" % table, text):
            launched.add(table)
    assert len(kernels) > 70, len(kernels)
    assert not sorted(kernels - launched), "kernels that no hipLaunchKernelGGL names: %s" % sorted(kernels - launched)
