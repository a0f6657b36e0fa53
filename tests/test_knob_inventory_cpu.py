"""CPU: every DSTAGNN_* environment variable the library reads is accounted for.

The rule ("Environment variables"): a variable read by dstagnn_drought_amd/csrc is
either a PATH SWITCH, which selects different code and therefore has a row in
tests/test_gpu_knobs.py::test_knob_path_vs_oracle, or a TOOL OVERRIDE, a debug / logging /
tuning value that a file kept under tools/ sets (TOOL_OVERRIDES below).  A switch of neither
kind is deleted together with the code only it reaches.  The library reads the environment only
through env_flag / env_int / env_str of common.hpp, which is what this test scans for."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dstagnn_drought_amd", "csrc")

# debug, logging and tuning values (set by hand or by the scripts under tools/); the three
# DSTAGNN_DEBUG_* probes also have rows in test_knob_path_vs_oracle
TOOL_OVERRIDES = (
    "DSTAGNN_GEMM_LOG",         # one "[gemm]" line per launch
    "DSTAGNN_GEMM_CFG",         # forces the tile configuration (tools/gemm_sweep.py)
    "DSTAGNN_GEMM_SPLITK",      # forces the split-K factor
    "DSTAGNN_GEMM_SKINNY",      # =0: the tiled kernel for the skinny shapes (tools/skinny_probe.sh)
    "DSTAGNN_SKINNY_KPW",       # k per wave of the skinny kernel
    "DSTAGNN_SKINNY_FOLD1_KB",  # one- / two-level fold threshold of the skinny kernel
    "DSTAGNN_SKINNY_STOP",      # stops the skinny kernel after a phase (tools/skinny_probe.sh)
    "DSTAGNN_HOST_PROFILE",     # host-side issue timing per stage
    "DSTAGNN_DEBUG_STREAMS",
    "DSTAGNN_DEBUG_MAIN_DELAY_US",
    "DSTAGNN_DEBUG_SIDE_DELAY_US",
)

READ = re.compile(r'\benv_(?:flag|int|str)\(\s*"(DSTAGNN_[A-Z0-9_]+)"')


def _sources():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".hpp", ".cpp", ".h")):
            with open(os.path.join(CSRC, f)) as fh:
                yield f, fh.read()


def _names_read():
    names = set()
    for _, text in _sources():
        names.update(READ.findall(text))
    return names


def _knob_rows():
    """The variable names of test_knob_path_vs_oracle's parameter table, read from the source
    of tests/test_gpu_knobs.py."""
    with open(os.path.join(ROOT, "tests", "test_gpu_knobs.py")) as fh:
        tree = ast.parse(fh.read())
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == "test_knob_path_vs_oracle":
            for dec in node.decorator_list:
                if isinstance(dec, ast.Call) and getattr(dec.func, "attr", "") == "parametrize":
                    rows = ast.literal_eval(dec.args[1])
                    return {env.split("=", 1)[0] for env, _cfg, _b in rows}
    raise AssertionError("test_knob_path_vs_oracle's parameter table not found")


def test_environment_is_read_through_the_helpers_only():
    bare = [f for f, text in _sources() if f != "common.hpp" and re.search(r"\bgetenv\s*\(", text)]
    assert not bare, f"bare getenv( outside common.hpp: {bare}"
    with open(os.path.join(CSRC, "common.hpp")) as fh:
        assert len(re.findall(r"\bgetenv\s*\(", fh.read())) == 1, "common.hpp: one getenv, inside env_str"


def test_every_variable_read_is_a_tested_path_switch_or_a_tool_override():
    read, rows = _names_read(), _knob_rows()
    assert read, "no env_flag / env_int / env_str call found: the scan is broken"
    stray = sorted(read - rows - set(TOOL_OVERRIDES))
    assert not stray, f"read by the library, but neither a test_knob_path_vs_oracle row nor a tool override: {stray}"


def test_no_stale_entry_in_either_list():
    read, rows = _names_read(), _knob_rows()
    assert len(set(TOOL_OVERRIDES)) == len(TOOL_OVERRIDES)
    gone = sorted((rows | set(TOOL_OVERRIDES)) - read)
    assert not gone, f"listed, but no longer read by the library: {gone}"

