"""fcg_tsi_capacity on the device against the extended-precision capacity of thermo_ref.py.

Criterion: the one of the regime tests (regimes_util.judge; the reason for its factor is in the
docstring of test_evaluate_regimes.py), with the float64 numpy restatement thermo_ref.capacity_f64 in
the oracle's place: with both measures e_n and e_c (element_ref.err_norm / err_comp against the scale
sum |capa w det J N_a N_b|),

    e(device) <= 4 * max(e(restatement), e_A(restatement)),

e_A the restatement's error in the benign case on the same mesh.  Each case prints "REGIMES {json}".

Meshes (the smallest at which the kernel can still go wrong):
  h8, h8r      hex8 (3,3,3), jitter 0.1, as a BoxMesh and as Discretization.renumbered: an interior
               node with 8 elements and 27 neighbours
  h27          hex27 (2,2,2): the 125-entry row the LDS row image is sized for
  h27_rank0/1  hex27 (2,2,4) over 2 ranks: ghost columns, owned rows beside ghosts
Regimes: the geometric ones of test_tsi_regimes.py that touch det J (D_1e4_rotated, H_thin, micro).
"""

import functools
import importlib

import numpy as np
import pytest

import regimes_util
import thermo_ref as th
from element_ref import EXTENDED
from regimes_util import _entry
from thermo_ref import MAT, MESHES, REGIMES, mesh_of

fcg = importlib.import_module("4c_amd").fcg
torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not EXTENDED, reason="np.longdouble has no 64-bit significand here")]

CAPA = 3.5e2


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _table(mesh):
    return np.where(np.arange(mesh.n_ele) % 3 == 0, CAPA, 7.25 * CAPA)


@functools.lru_cache(maxsize=None)
def _problem(name, regime, table=False):
    mesh, g = mesh_of(name, regime)
    capa = _table(mesh) if table else CAPA
    C, S, mindet = th.capacity(mesh, g, capa)
    assert mindet > 0
    if regime == "micro":
        assert 1e-16 < mindet < 1e-14, mindet
    return {"C": _entry(C, S, th.capacity_f64(mesh, g, capa))}


def _tev(name, regime="A"):
    _dev()
    mesh, g = mesh_of(name, regime)
    return fcg.TsiEvaluator(mesh, MAT["youngs"], MAT["poisson"], MAT["thexpans"], MAT["inittemp"],
                            MAT["conduct"], graph=g), mesh, g


def _nan(n):
    return torch.full((int(n),), float("nan"), dtype=torch.float64, device=_dev())


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("name", list(MESHES))
def test_capacity_against_longdouble(name, regime):
    tev, mesh, g = _tev(name, regime)
    a = tev.capacity(CAPA, out=_nan(g.nnz_tt))      # OVERWRITE over NaN leaves none
    b = tev.capacity(CAPA, out=_nan(g.nnz_tt))
    tev.close()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)                        # two calls, the same bits
    regimes_util.judge(f"capacity/{name}/{regime}", _problem(name, regime), _problem(name, "A"),
                       {"C": a.cpu().numpy()}, {})


@pytest.mark.parametrize("name", list(MESHES))
def test_element_table(name):
    tev, mesh, g = _tev(name)
    tab = _table(mesh)
    assert len(set(tab)) == 2
    got = tev.capacity(0.0, ele_capa=tab, out=_nan(g.nnz_tt))   # capa is ignored beside a table
    uni = tev.capacity(CAPA)
    same = tev.capacity(-1.0, ele_capa=np.full(mesh.n_ele, CAPA))
    tev.close()
    assert torch.equal(uni, same)                   # a table of equal values is the uniform call
    regimes_util.judge(f"capacity_table/{name}", _problem(name, "A", True), _problem(name, "A", True),
                       {"C": got.cpu().numpy()}, {})


@pytest.mark.parametrize("name", ["h8r", "h27_rank1"])
def test_accumulate_adds(name):
    tev, mesh, g = _tev(name)
    one = tev.capacity(CAPA)
    acc = tev.capacity(CAPA, mode=fcg.ACCUMULATE)   # onto zeros
    assert torch.equal(acc, one)
    tev.capacity(CAPA, mode=fcg.ACCUMULATE, out=acc)
    tev.close()
    eps = np.finfo(np.float64).eps
    assert bool(((acc - 2 * one).abs() <= 4 * eps * one.abs()).all())


def test_argument_errors():
    tev, mesh, g = _tev("h8")
    out = _nan(g.nnz_tt)
    for capa in (0.0, -2.0, float("nan")):
        with pytest.raises(fcg.FcgError) as e:
            tev.capacity(capa, out=out)
        assert e.value.code == 3 and "capa" in str(e.value)
    tab = np.full(mesh.n_ele, CAPA)
    tab[3] = 0.0
    with pytest.raises(fcg.FcgError) as e:
        tev.capacity(CAPA, ele_capa=tab, out=out)
    assert e.value.code == 3 and "ele_capa[3]" in str(e.value)
    tab[3] = -1.0
    with pytest.raises(fcg.FcgError) as e:
        tev.capacity(CAPA, ele_capa=tab, out=out)
    assert e.value.code == 3 and "ele_capa[3]" in str(e.value)
    with pytest.raises(fcg.FcgError) as e:
        tev.capacity(CAPA, mode=7, out=out)
    assert e.value.code == 3
    assert torch.isnan(out).all()                   # a refused call writes nothing
    tev.close()


def test_mirrored_mesh_reports_the_element():
    """x -> -x turns every element inside out: det J < 0 at every Gauss point, an ordinary error
    return with the lowest element GID."""
    _dev()
    box, g = mesh_of("h8")
    m = type("Mirrored", (), {})()
    for key in ("celltype", "n_ele", "n_node", "n_rows", "n_cols", "ele_nodes", "node_dof_row", "node_dof_col"):
        setattr(m, key, getattr(box, key))
    m.node_x = np.ascontiguousarray(np.asarray(box.node_x) * np.array([-1.0, 1.0, 1.0]))
    m.ele_gid = np.ascontiguousarray(np.asarray(box.ele_gid) + 40, dtype=np.int32)
    tev = fcg.TsiEvaluator(m, MAT["youngs"], MAT["poisson"], MAT["thexpans"], MAT["inittemp"], MAT["conduct"],
                           graph=g)
    with pytest.raises(fcg.FcgError) as e:
        tev.capacity(CAPA)
    tev.close()
    assert e.value.code == fcg.FCG_ERR_NODAL_DETJ
    assert e.value.bad_ele_gid == int(m.ele_gid.min()) == 40
