"""Records the fixtures of the save-plan tests from a PARENT build of the library.

  python tools/record_save_plan.py sizes PARENT/libdstagnn.so     (host only)
      -> tests/golden/save_plan_parent_sizes.json: save / scratch / work bytes and the path bits of
         every row of tests/test_forward_only_cpu.py::test_workspace_holds_no_backward_state and
         of the two dth_base rows
  LD_LIBRARY_PATH=PARENT DSTAGNN_EXT=PARENT/_C.so python tools/record_save_plan.py hashes [OUT]
      -> tests/golden/save_plan_parent_hashes.json: sha256 of out, re_at, grad_x and every parameter
         gradient on the default path (tests/test_gpu_save_plan.py BIT_CASES), from two fresh blocks
         each; a tensor whose two runs differ is listed under "unreproducible" and carries no hash
"""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def sizes(lib_path):
    import test_forward_only_cpu as fo
    lib = ctypes.CDLL(lib_path)
    rows = {}
    for name, first, B in fo.size_rows():
        d = fo._dims(name, first, B)
        rows[fo.row_key(name, first, B)] = dict(zip(("paths", "save", "scratch", "work"), fo.plan_of(lib, d)))
    with open(os.path.join(GOLDEN, "save_plan_parent_sizes.json"), "w") as f:
        json.dump({"lib_sha256": hashlib.sha256(open(lib_path, "rb").read()).hexdigest()[:16], "rows": rows}, f,
                  indent=0, sort_keys=True)
    print(f"{len(rows)} rows")


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def hashes(out_path):
    import test_gpu_save_plan as sp
    rec = {"cases": {}, "unreproducible": {}}
    for case in sp.BIT_CASES:
        a, b = sp.run_case(*case), sp.run_case(*case)
        assert a.keys() == b.keys()
        same = {k: sha(a[k]) == sha(b[k]) for k in a}
        rec["cases"][sp.case_id(*case)] = {k: sha(a[k]) for k in a if same[k]}
        rec["unreproducible"][sp.case_id(*case)] = sorted(k for k in a if not same[k])
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
    print(json.dumps(rec["unreproducible"]), "RECORD_OK")


if __name__ == "__main__":
    if sys.argv[1] == "sizes":
        sizes(sys.argv[2])
    else:
        hashes(sys.argv[2] if len(sys.argv) > 2 else os.path.join(GOLDEN, "save_plan_parent_hashes.json"))
