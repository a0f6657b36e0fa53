"""CPU: every DSTAGNN_* environment variable the library reads is accounted for.

The rule ("Environment variables"): a variable read by dstagnn_drought_amd/csrc is
either a PATH SWITCH, which selects different code and therefore has a row in
tests/test_gpu_knobs.py::test_knob_path_vs_oracle, or a TOOL OVERRIDE, a debug / logging /
tuning value that a file kept under tools/ sets (TOOL_OVERRIDES below).  A switch of neither
kind is deleted together with the code only it reaches.  The library reads the environment only
through env_flag / env_int / env_str of common.hpp, which is what this test scans for.  The
table of DESIGN.md §9, the third copy of the list, is held to the same set."""
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


def _design_table_names():
    """The back-quoted DSTAGNN_* tokens of DESIGN.md §9's table rows (the lines that start with
    "|" between the "## 9." heading and "### Experiment code removed"; the prose is not read)."""
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        text = fh.read()
    head = re.search(r"^## 9\..*$", text, re.M)
    assert head, "DESIGN.md: the '## 9.' heading not found"
    end = text.find("### Experiment code removed", head.end())
    assert end > 0, "DESIGN.md: '### Experiment code removed' not found after '## 9.'"
    rows = [l for l in text[head.end():end].splitlines() if l.startswith("|")]
    return [t for l in rows for t in re.findall(r"`([^`]*)`", l) if "DSTAGNN_" in t]


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


def test_design_table_lists_exactly_the_variables_read():
    tokens = _design_table_names()
    assert tokens, "DESIGN.md §9: no DSTAGNN_* token in the table rows: the scan is broken"
    short = [t for t in tokens if not re.fullmatch(r"DSTAGNN_[A-Z0-9_]+", t)]
    assert not short, f"DESIGN.md §9: one full variable name per back-quoted token, got {short}"
    assert len(set(tokens)) == len(tokens), f"DESIGN.md §9: a variable listed twice: {sorted(tokens)}"
    read = _names_read()
    assert set(tokens) == read, (f"DESIGN.md §9 table vs the library: only in the table "
                                 f"{sorted(set(tokens) - read)}, only read {sorted(read - set(tokens))}")

