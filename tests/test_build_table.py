"""CPU-only checks of rl_on_manifold_amd/build.py: the table of the six libraries, and the rule that rebuilds a library for its
units and what they include.  Nothing is compiled and no source is edited."""
import os

import pytest

import abi_tools as abi

CSRC_FILES = """
atacom_capi.cpp atacom_capi_common.h atacom_chart.h atacom_chart.hip atacom_chart_group.h atacom_chart_iiwa.hip
atacom_circle.hip atacom_dynamics.h atacom_dynamics_link.h atacom_envs.h atacom_iiwa.hip atacom_iiwa_dyn.hip
atacom_iiwa_dyn_chart.hip atacom_iiwa_dyn_f64.hip atacom_iiwa_f64.hip atacom_iiwa_group.h atacom_iiwa_group.hip
atacom_iiwa_inertia.h atacom_kernels.h atacom_linalg.h atacom_mlp_host.h atacom_noise_iiwa.hip atacom_noise_iiwa_f64.hip
atacom_noise_planar.hip atacom_ops.h atacom_ops_impl.h atacom_planar.hip atacom_point.h atacom_point.hip
atacom_point_capi.cpp atacom_point_compact.h atacom_point_compact.hip atacom_point_compact_capi.cpp
atacom_point_compact_ops.h atacom_point_handle.h atacom_point_ops.h atacom_point_policy.h atacom_point_policy.hip
atacom_point_policy_capi.cpp atacom_point_policy_ops.h atacom_point_vec.h atacom_point_vec.hip atacom_point_vec_capi.cpp
atacom_point_vec_ops.h atacom_policy.h atacom_quad.h
""".split()
CSRC_RETURNS_FILES = ['atacom_returns.h', 'atacom_returns.hip', 'atacom_returns_capi.cpp']
# name: (library, the variable that redirects it, directory, units); the main library's units are the rest of csrc/
TABLE = {
    'hip': ('libatacom_hip.so', 'ATACOM_LIB_OUT', 'csrc', None),
    'point': ('libatacom_point.so', 'ATACOM_POINT_LIB_OUT', 'csrc', ['atacom_point.hip', 'atacom_point_capi.cpp']),
    'point_policy': ('libatacom_point_policy.so', 'ATACOM_POINT_POLICY_LIB_OUT', 'csrc',
                     ['atacom_point_policy.hip', 'atacom_point_policy_capi.cpp']),
    'point_compact': ('libatacom_point_compact.so', 'ATACOM_POINT_COMPACT_LIB_OUT', 'csrc',
                      ['atacom_point_compact.hip', 'atacom_point_compact_capi.cpp']),
    'point_vec': ('libatacom_point_vec.so', 'ATACOM_POINT_VEC_LIB_OUT', 'csrc', ['atacom_point_vec.hip', 'atacom_point_vec_capi.cpp']),
    'returns': ('libatacom_returns.so', 'ATACOM_RETURNS_LIB_OUT', 'csrc_returns', ['atacom_returns.hip', 'atacom_returns_capi.cpp']),
}
# what each later library added: its units, its private headers and its public header
OWN = {
    'point_policy': {'atacom_point_policy.hip', 'atacom_point_policy_capi.cpp', 'atacom_point_policy.h', 'atacom_point_policy_ops.h',
                     'atacom_point_policy_hip.h'},
    'point_compact': {'atacom_point_compact.hip', 'atacom_point_compact_capi.cpp', 'atacom_point_compact.h',
                      'atacom_point_compact_ops.h', 'atacom_point_compact_hip.h'},
    'point_vec': {'atacom_point_vec.hip', 'atacom_point_vec_capi.cpp', 'atacom_point_vec.h', 'atacom_point_vec_ops.h',
                  'atacom_point_vec_hip.h'},
    'returns': set(CSRC_RETURNS_FILES) | {'atacom_returns_hip.h'},
}
# file: which of hip, point, point_policy, point_compact, point_vec, returns it makes stale
STALE = {
    'atacom_capi.cpp': '100000', 'atacom_capi_common.h': '111111', 'atacom_linalg.h': '111110', 'atacom_kernels.h': '111110',
    'atacom_hip.h': '101100',
    'atacom_iiwa_group.h': '100000', 'atacom_ops.h': '100000', 'atacom_ops_impl.h': '100000', 'atacom_mlp_host.h': '101100',
    'atacom_point.h': '011110', 'atacom_point_handle.h': '011110', 'atacom_point_hip.h': '011110', 'atacom_point_ops.h': '010000',
    'atacom_point_policy.h': '001100', 'atacom_point_policy_ops.h': '001100', 'atacom_point_policy_hip.h': '001100',
    'atacom_point_policy.hip': '001000',
    'atacom_point_compact.h': '000100', 'atacom_point_compact_ops.h': '000100', 'atacom_point_compact_hip.h': '000100',
    'atacom_point_compact_capi.cpp': '000100',
    'atacom_point_vec.h': '000010', 'atacom_point_vec_ops.h': '000010', 'atacom_point_vec_hip.h': '000010',
    'atacom_point_vec.hip': '000010', 'atacom_point_vec_capi.cpp': '000010',
    'atacom_returns.h': '000001', 'atacom_returns.hip': '000001', 'atacom_returns_capi.cpp': '000001',
    'atacom_returns_hip.h': '000001',
}


def test_the_table_is_the_six_libraries_with_their_units():
    from rl_on_manifold_amd import build
    assert list(build.TARGETS) == list(TABLE)
    assert sorted(f for f in os.listdir(build.CSRC) if f.endswith(('.h', '.hip', '.cpp'))) == sorted(CSRC_FILES)
    assert sorted(f for f in os.listdir(build.CSRC_RETURNS) if f.endswith(('.h', '.hip', '.cpp'))) == CSRC_RETURNS_FILES
    for name, (lib, env, directory, units) in TABLE.items():
        t = build.TARGETS[name]
        assert os.path.basename(t.lib) == lib or os.environ.get(env), name
        assert t.dir == os.path.join(build.HERE, directory) and t.dir in (build.CSRC, build.CSRC_RETURNS), name
        assert t.units == units or name == 'hip', name
        assert t.tuning == (name == 'hip')
    # the main library: every other unit of csrc/, the group kernels' source first and the C ABI last
    assert build.TARGETS['hip'].units is build.UNITS and build.TARGETS['hip'].lib == build.LIB
    assert len(build.UNITS) == 14 and build.UNITS[0] == 'atacom_iiwa.hip' and build.UNITS[-1] == 'atacom_capi.cpp'
    assert sorted(build.UNITS) == sorted(f for f in CSRC_FILES if not f.endswith('.h') and not f.startswith('atacom_point'))
    units = [u for t in build.TARGETS.values() for u in t.units]
    assert len(units) == len(set(units)) == 24
    # nothing that the main library compiles names the collision-avoidance task (its kernel census is pinned,
    # tests/test_policy_kernel_resources.py)
    for f in CSRC_FILES:
        if not f.startswith('atacom_point'):
            assert 'atacom_point' not in open(os.path.join(build.CSRC, f)).read(), f


def test_a_touched_file_makes_exactly_the_libraries_that_include_it_stale(monkeypatch):
    from rl_on_manifold_amd import build
    touched = abi.fake_mtimes(monkeypatch, build)
    assert [build.stale(name) for name in build.TARGETS] == [False] * 6
    for name, want in STALE.items():
        touched[:] = [name]
        assert ''.join('01'[build.stale(n)] for n in build.TARGETS) == want, name
        assert any(os.path.exists(os.path.join(d, name)) for d in (build.CSRC, build.CSRC_RETURNS, abi.INCLUDE)), name


def test_own_files_and_borrowed_headers():
    from rl_on_manifold_amd import build
    src = {name: {os.path.basename(p) for p in build.sources(t)} for name, t in build.TARGETS.items()}
    lent = {('point_policy', 'point_compact'): {'atacom_point_policy.h', 'atacom_point_policy_ops.h', 'atacom_point_policy_hip.h'}}
    for mine, own in OWN.items():
        assert own <= src[mine], mine
        for other in src:                            # editing a library's files makes no other library stale ...
            if other != mine:
                assert own & src[other] == lent.get((mine, other), set()), (mine, other)
    # ... and what a library borrows makes it stale: the handle, the environment, the policy kernel's header and validator
    assert {'atacom_point_handle.h', 'atacom_point.h', 'atacom_point_policy.h', 'atacom_point_policy_ops.h', 'atacom_policy.h',
            'atacom_point_compact_hip.h'} <= src['point_compact']
    assert {'atacom_point_handle.h', 'atacom_point.h', 'atacom_point_hip.h', 'atacom_point_vec_hip.h', 'atacom_kernels.h'} <= src['point_vec']
    assert not {'atacom_point_policy.h', 'atacom_point_policy_ops.h', 'atacom_point_compact.h', 'atacom_point_compact_ops.h'} & \
        src['point_vec']
    assert src['returns'] == OWN['returns'] | {'atacom_capi_common.h'}
    for name in src:
        assert name == 'returns' or not any('returns' in f for f in src[name]), name


def test_the_include_closure(tmp_path):
    """sources() on files made here: no compiler and none of the repository's files."""
    from rl_on_manifold_amd import build
    (tmp_path / 'src' / 'sub').mkdir(parents=True)
    (tmp_path / 'include').mkdir()
    files = {'src/a.hip': '#include <vector>\n#include "b.h"\n  #  include "sub/c.h"\n',
             'src/b.h': '#include "../include/pub.h"\n',
             'src/sub/c.h': '#if 0\n#include "../off.h"\n#endif\n// #include "gone.h"\n',
             'src/off.h': '', 'src/unused.h': '', 'include/pub.h': '#include <stdint.h>\n', 'src/a_capi.cpp': '#include "b.h"\n'}
    for name, text in files.items():
        (tmp_path / name).write_text(text)
    target = build.Target(str(tmp_path / 'liba.so'), str(tmp_path / 'src'), ['a.hip', 'a_capi.cpp'], False)
    got = build.sources(target)
    assert got[:2] == [str(tmp_path / 'src' / u) for u in target.units]
    assert sorted(os.path.relpath(p, str(tmp_path)) for p in got) == ['include/pub.h', 'src/a.hip', 'src/a_capi.cpp', 'src/b.h',
                                                                      'src/off.h', 'src/sub/c.h']
    (tmp_path / 'src' / 'b.h').write_text('#include "missing.h"\n')
    with pytest.raises(FileNotFoundError, match=r'b\.h includes "missing\.h"'):
        build.sources(target)
