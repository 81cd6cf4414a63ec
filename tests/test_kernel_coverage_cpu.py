"""Kernel launch coverage as a standing contract (no GPU): tests/kernel_coverage.tsv names, for every kernel instantiation
the library compiles, the test files that launch it -- taken from a kernel-trace audit of the suite (tools/kernel_coverage.py,
profiles/kernel_coverage.md) -- or the documented reason it cannot be held to a reference.  Adding or dropping an instantiation
fails here until the table says who tests it; DESIGN.md ("Kernel launch coverage") tells how to refresh the table."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "kernel_coverage.tsv")


def _tool():
    spec = importlib.util.spec_from_file_location("_anyloc_kernel_coverage", os.path.join(ROOT, "tools", "kernel_coverage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def kc():
    return _tool()


@pytest.fixture(scope="module")
def rows(kc):
    rows = kc.read_tsv(TABLE)
    assert rows and all(len(r) == 4 for r in rows), "four tab-separated columns: kernel, source, test | exempt, witnesses | reason"
    return rows


@pytest.fixture(scope="module")
def compiled(kc):
    missing = kc.tools_missing()
    if missing:
        pytest.skip("ROCm binaries that read the library's device code are missing: " + ", ".join(missing))
    return kc.compiled()                                  # (a library that is not built is an error, not a skip)


def test_the_table_lists_exactly_the_compiled_kernels(kc, rows, compiled):
    names = [r[0] for r in rows]
    assert len(set(names)) == len(names), "a kernel is listed twice"
    table, built = set(names), set(compiled)
    new, gone = sorted(built - table), sorted(table - built)
    assert not new and not gone, (f"{len(new)} compiled kernel(s) have no row in tests/kernel_coverage.tsv (which test launches them?): {new[:8]}; "
                                  f"{len(gone)} row(s) name a kernel that is no longer compiled: {gone[:8]}")
    if "?" not in compiled.values():                      # (the objects are there: their names give the source files)
        wrong = [(r[0], r[1], compiled[r[0]]) for r in rows if compiled[r[0]] != r[1]]
        assert not wrong, wrong[:8]


def test_every_witness_is_a_test_file(rows):
    for name, _, kind, wit in rows:
        assert kind in ("test", "exempt"), (name, kind)
        if kind == "test":
            files = wit.split(",")
            assert files and all(f.startswith("test_gpu_") and f.endswith(".py") and os.path.isfile(os.path.join(ROOT, "tests", f))
                                 for f in files), (name, wit)


def test_only_the_two_study_families_are_exempt(kc, rows):
    exempt = [r for r in rows if r[2] == "exempt"]
    assert len(exempt) <= kc.EXEMPT_MAX == 14
    for name, _, _, reason in exempt:
        assert kc.exempt_reason(name) is not None, f"{name} is neither gemm_nt_kernel with ablation 1 - 4 nor fused3_kernel with GV != 0"
        assert reason.strip() and reason != "NEVER"


def test_names_normalise_alike_from_both_demanglers(kc):
    """a kernel descriptor symbol through c++filt and a kernel trace's name give the same string"""
    want = "screen_rescore_sliced_kernel<8>"
    assert kc.normalise("void anyloc::(anonymous namespace)::screen_rescore_sliced_kernel<8>(float const*, float const*, long, long, int, "
                        "int const*, int const*, int, float const*, float const*, float const*, float*) [clone .kd]") == want
    assert kc.normalise("void anyloc::(anonymous namespace)::screen_rescore_sliced_kernel<8>(float const*, float const*, long, long, int, "
                        "int const*, int const*, int, float const*, float const*, float const*, float*)") == want
    assert kc.normalise("anyloc::(anonymous namespace)::gemm_screen_kernel(anyloc::H3Problem, int, int) [clone .kd]") == "gemm_screen_kernel"
    assert kc.normalise("void anyloc::fused3_kernel<12, 8, (bool)0, 1u>(float const*)") == "fused3_kernel<12, 8, false, 1>"
    assert kc.exempt_reason("fused3_kernel<12, 8, false, 1>") and not kc.exempt_reason("fused3_kernel<12, 8, false, 0>")
    assert kc.exempt_reason("gemm_nt_kernel<128, 128, 2, 2, 32, 2, 0, false, true, 4>")
    assert not kc.exempt_reason("gemm_nt_kernel<128, 128, 2, 2, 32, 2, 0, false, true, 8>")
