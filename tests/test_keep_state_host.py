"""`keep_state` of OscillinkLattice.append / remove / update, as far as it goes without a device:
osc_carry_state is declared, exported and bound; it refuses NULL arguments before any device work; the three methods take
`keep_state` by keyword only, default False; and the maps they hand to `_become` follow the rule
U_new[a] = U_old[src[a]] where src[a] >= 0, else Y_new[a]."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from oscillink_amd import _build, _native

    _build.build()
    return _native.lib()


def test_carry_state_is_declared_exported_and_bound(lib):
    from oscillink_amd import _native as nat

    txt = open(os.path.join(ROOT, "include", "oscillink_hip.h")).read()
    decl = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int osc_carry_state\(osc_handle dst, osc_handle src, "
                     r"const int32_t\* src_row_of_dst\);", txt, re.S)
    assert decl, "osc_carry_state is not declared with its comment"
    comment = " ".join(decl.group(1).split())
    assert "lat.U" in comment and "osc_get_U" in comment and "osc_set_U" in comment  # what it replaces
    assert nat.SIGNATURES["osc_carry_state"] == (ctypes.c_int, [nat.Handle, nat.Handle, nat.c_i32p])
    assert hasattr(lib, "osc_carry_state")
    # (the counters keep their nine fields: the carry adds none)
    assert len(nat.Counters._fields_) == 9


def test_null_arguments_are_refused_without_a_device(lib):
    from oscillink_amd import _native as nat

    m = np.zeros(4, dtype=np.int32)
    fake = nat.Handle(0)
    assert lib.osc_carry_state(None, None, None) == nat.OSC_E_INVALID
    assert lib.osc_carry_state(None, None, nat.i32(m)) == nat.OSC_E_INVALID
    assert lib.osc_carry_state(fake, fake, nat.i32(m)) == nat.OSC_E_INVALID
    assert b"osc_carry_state" in lib.osc_last_error(None)


@pytest.mark.parametrize("name", ["append", "remove", "update"])
def test_keep_state_is_keyword_only_and_off_by_default(name):
    from oscillink_amd import OscillinkLattice

    p = inspect.signature(getattr(OscillinkLattice, name)).parameters["keep_state"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


def _expected(U_old, Y_new, src):
    return np.where((src >= 0)[:, None], U_old[np.maximum(src, 0)], Y_new)


def test_the_map_helpers():
    from oscillink_amd import lattice as lt

    a = lt._state_map_append(5, 3)
    assert a.dtype == np.int32 and a.tolist() == [0, 1, 2, 3, 4, -1, -1, -1]
    keep = np.array([False, True, True, False, True, False])
    r = lt._state_map_remove(keep)
    assert r.dtype == np.int32 and r.tolist() == [1, 2, 4]
    u = lt._state_map_update(6, np.array([5, 0, 3], dtype=np.int64))
    assert u.dtype == np.int32 and u.tolist() == [-1, 1, 2, -1, 4, -1]
    for m in (a, r, u):
        assert m.flags["C_CONTIGUOUS"]


class _Recorder:
    """An OscillinkLattice without a handle whose `_become` records its arguments: what the three methods compute on the
    host up to the native calls."""

    def __new__(cls, N, D):
        from oscillink_amd import OscillinkLattice

        class Rec(OscillinkLattice):
            def __del__(self):
                pass

            def _become(self, op, cannot, create, rows, N_new, B_new, chain_nodes, state_map=None):
                self.calls.append((op, rows, N_new, state_map))

        lat = object.__new__(Rec)
        lat._h = None
        lat.N, lat.D = N, D
        lat._B = np.ones(N, dtype=np.float32)
        lat._chain_nodes = None
        lat.calls = []
        return lat


def test_without_keep_state_no_map_is_built():
    lat = _Recorder(7, 3)
    rows = np.zeros((2, 3), dtype=np.float32)
    lat.append(rows)
    lat.remove([1, 2])
    lat.update([0, 6], rows)
    lat.append(rows, keep_state=False)
    assert [c[0] for c in lat.calls] == ["append", "remove", "update", "append"]
    assert all(c[3] is None for c in lat.calls)


def test_append_map_names_the_old_rows_then_fresh_ones():
    N, D, M = 7, 3, 4
    lat = _Recorder(N, D)
    rng = np.random.default_rng(0)
    U, Y, Ynew = (rng.standard_normal(s).astype(np.float32) for s in ((N, D), (N, D), (M, D)))
    ids = lat.append(Ynew, keep_state=True)
    (op, rows, N_new, src), = lat.calls
    assert (op, rows, N_new) == ("append", M, N + M) and ids.tolist() == list(range(N, N + M))
    assert src.dtype == np.int32 and src.shape == (N + M,)
    assert src.tolist() == list(range(N)) + [-1] * M
    want = np.concatenate([U, Ynew])
    assert np.array_equal(_expected(U, np.concatenate([Y, Ynew]), src), want)


@pytest.mark.parametrize("ids", [[3], [0], [8], [8, 0], [5, 2, 5, 2, 2], [7, 8, 0, 1, 4, 4]],
                         ids=["one", "first", "last", "last_and_first", "duplicates", "unordered_with_duplicates"])
def test_remove_map_names_the_kept_rows_in_order(ids):
    N, D = 9, 2
    lat = _Recorder(N, D)
    U = np.random.default_rng(1).standard_normal((N, D)).astype(np.float32)
    new_id_of_old = lat.remove(ids, keep_state=True)
    (op, rows, N_new, src), = lat.calls
    gone = sorted(set(ids))
    assert (op, rows, N_new) == ("remove", len(gone), N - len(gone))
    assert src.dtype == np.int32 and src.tolist() == [i for i in range(N) if i not in gone]
    assert (src >= 0).all()  # a removal has no fresh row
    # the two views of one renumbering agree: row new_id_of_old[o] of the lattice afterwards is old row o
    for o in range(N):
        assert (new_id_of_old[o] == -1) == (o in gone)
        if o not in gone:
            assert src[new_id_of_old[o]] == o
    assert np.array_equal(_expected(U, np.zeros((N_new, D), np.float32), src), np.delete(U, gone, axis=0))


@pytest.mark.parametrize("ids", [[4], [0], [8], [8, 0, 4], [6, 1, 3, 2]],
                         ids=["one", "first", "last", "last_first_middle", "unordered"])
def test_update_map_marks_the_replaced_rows_fresh(ids):
    N, D = 9, 2
    lat = _Recorder(N, D)
    rng = np.random.default_rng(2)
    U, Y = (rng.standard_normal((N, D)).astype(np.float32) for _ in range(2))
    Ynew = rng.standard_normal((len(ids), D)).astype(np.float32)
    out = lat.update(np.asarray(ids, dtype=np.int16), Ynew, keep_state=True)
    (op, rows, N_new, src), = lat.calls
    assert (op, rows, N_new) == ("update", len(ids), N) and out.tolist() == ids
    assert src.dtype == np.int32 and src.shape == (N,)
    assert src.tolist() == [-1 if i in ids else i for i in range(N)]
    Y2, want = Y.copy(), U.copy()
    Y2[ids] = Ynew
    want[ids] = Ynew  # a replaced row starts at its NEW anchor, in the order the rows were given
    assert np.array_equal(_expected(U, Y2, src), want)
