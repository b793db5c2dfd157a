"""The table of per-model facts (extendedrtirtmodeling.jl_amd/csrc/erm_model.hpp) on the CPU: the header the host side reads is compiled by g++ with
UndefinedBehaviorSanitizer, AddressSanitizer and -ftrapv into tests/model_check.cpp (a stand-alone program), which checks the N x J layout helpers, the parameter
block's field table, beta's packing and the offsets loglik_kernel reads, and prints the traits, every derived width, length and offset and the blocks of every trace
for a grid of small (N, J, F) (N = 1, J = 1 and F = 0 among them).  The output is compared with the shapes the reference recorded in
tests/golden/*.npz, with the Python side's copy of the table (_lib.MODEL_TRAITS), and with the invariants the engine relies on."""
import os
import subprocess

import numpy as np
import pytest

import parity_util as pu

pkg = pu.ge.load_package()
L = pkg._lib
INT_KEYS = ("rt", "rho", "sees_x", "gen", "kernel_feat", "nbeta", "nq", "sigp_off", "qr_head", "item", "nu_len", "ra", "rtw", "qr", "ll", "sum_theta", "sum_zeta", "sum_nu", "sum_len")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """{(model, N, J, F): {key: value}} as tests/model_check.cpp prints it; the program's own checks (layout helpers, out-of-range lookups, the engine's limits) passed."""
    exe = str(tmp_path_factory.mktemp("model") / "model_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-ftrapv", "-I", pu.GEOMETRY_INC, "-I", os.path.join(pu.ROOT, "include"),
                    os.path.join(pu.ROOT, "tests", "model_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "layout and range failures 0" in r.stderr, r.stderr[-4000:]
    out = {}
    for ln in r.stdout.splitlines():
        kv = dict(p.split("=", 1) for p in ln.split())
        row = {k: (int(v) if k in INT_KEYS else v) for k, v in kv.items() if k not in ("model", "N", "J", "F")}
        out[tuple(int(kv[k]) for k in ("model", "N", "J", "F"))] = row
    assert len(out) == 7 * 4 * 3 * 3 and {(0, 1, 1, 0), (2, 1, 1, 0), (3, 160, 7, 3)} <= set(out)
    return out


# the reference's recorded shapes at N = 160, J = 7, F = 3 (tests/golden/*.npz): width of qr, entries of init_beta (None: the file has init_rho instead)
GOLDEN_SHAPES = {"mlirt": (4, 4), "rtirt": (12, 8), "null": (12, 8), "cross": (11, None), "crossqr": (11, None), "latentqr": (169, 5), "latent": (9, 5)}


@pytest.mark.parametrize("name", sorted(pu.MODELS))
def test_table_gives_the_shapes_the_reference_recorded(table, name):
    z = np.load(os.path.join(pu.ROOT, "tests", "golden", f"{name}.npz"))
    N, J = z["Y"].shape
    F = 3
    assert (N, J) == (160, 7)
    t = table[(pu.MODELS[name], N, J, F)]
    qr_w, nb = GOLDEN_SHAPES[name]
    assert z["qr"].shape[1] == qr_w and z["ra"].shape[1] == N + 2 * J == 174 == t["ra"]
    if name == "crossqr":          # the fixture stores the prefix [rho; vec(Sigp)] of the J + 4 + N * J columns
        assert t["qr"] == J + 4 + N * J and t["qr"] - t["nu_len"] == qr_w
    else:
        assert t["qr"] == qr_w
    if nb is None:
        assert "init_beta" not in z.files and z["init_rho"].shape == (J,) and t["rho"] == 1 and t["nbeta"] == 0
    else:
        assert z["init_beta"].size == nb == t["nbeta"] and "init_rho" not in z.files and t["rho"] == 0
    assert ("logT" in z.files) == bool(t["rt"])
    assert (t["rtw"] == 174) == bool(t["rt"]) and t["rtw"] in (0, 174)
    assert ("X" in z.files) >= bool(t["sees_x"])          # (Null's fixture carries the X its generator made; the sampler ignores it)


def test_python_table_agrees_entry_for_entry(table):
    assert sorted(L.MODEL_TRAITS) == sorted(pu.MODELS.values()) == list(range(7))
    for (model, N, J, F), t in table.items():
        py = L.MODEL_TRAITS[model]
        assert (int(py.rt), int(py.rho), py.nu, int(py.sees_x), py.beta, py.gen) == (t["rt"], t["rho"], t["nu"], t["sees_x"], t["beta"], t["gen"]), model
        assert (L.nbeta(model, F), L.nu_len(model, N, J), L.kernel_feat(model, F)) == (t["nbeta"], t["nu_len"], t["kernel_feat"]), (model, N, J, F)
        assert int(np.prod(L.beta_shape(model, F), dtype=np.int64)) == t["nbeta"] or py.beta == "none"
    with pytest.raises(TypeError):
        L.MODEL_TRAITS[0] = None          # immutable
    with pytest.raises(AttributeError):
        L.MODEL_TRAITS[0].rt = True


def test_derived_widths_keep_their_invariants(table):
    for (model, N, J, F), t in table.items():
        key = (model, N, J, F)
        assert t["item"] == 4 * J + t["nq"], key
        assert t["ll"] == 1 and t["ra"] == N + 2 * J, key
        assert t["nq"] == t["sigp_off"] + 4 * t["rt"], key
        assert t["qr"] == t["qr_head"] + 4 * t["rt"] + t["nu_len"], key
        assert t["qr_head"] == (J if t["rho"] else t["nbeta"]), key
        # the kernels' small part differs from Post.qr's only where the kernels see fewer covariate columns than beta is reported over (Null)
        assert (t["sigp_off"] == t["qr_head"]) == (t["beta"] != "zero_pair" or F == 0), key
        # the summary vector: [item columns | theta | zeta | nu], the offsets increasing, an absent block at -1, the last block ending at the length
        blocks = [(t["sum_theta"], N), (t["sum_zeta"], N if t["rt"] else 0), (t["sum_nu"], t["nu_len"])]
        end = t["item"]
        for off, n in blocks:
            assert off == (end if n else -1), key
            end += n
        assert end == t["sum_len"], key
        assert (t["nu"] == "none") == (t["nu_len"] == 0) and t["kernel_feat"] == (F if t["sees_x"] else 0), key


def _blocks(text):
    """[(kind, ncol, col0, src, device_order)] of a trace as tests/model_check.cpp prints it ('-': no block)"""
    return [] if text == "-" else [(k, int(n), int(c), int(s), bool(int(d))) for k, n, c, s, d in (b.split(":") for b in text.split(";"))]


def test_blocks_tile_every_trace(table):
    """The blocks of each trace tile [0, trace_width) in order without gap or overlap, none is empty, there are at most four, and the widths they add up to are
    the ones the independent formulas give (ra = N + 2J, rt the same or nothing, qr = head + Sigp + nu; logLike is one column made of no block)."""
    for (model, N, J, F), t in table.items():
        key = (model, N, J, F)
        assert _blocks(t["blocks_ll"]) == [] and t["ll"] == 1, key
        for name, width in (("ra", N + 2 * J), ("rt", (N + 2 * J) * t["rt"]), ("qr", t["qr_head"] + 4 * t["rt"] + t["nu_len"])):
            end = 0
            blocks = _blocks(t["blocks_" + name])
            for kind, ncol, col0, src, dev in blocks:
                assert col0 == end and ncol > 0 and kind in "SCIZ", (key, name)
                end += ncol
            assert len(blocks) <= 4 and end == width, (key, name)
            assert end == t[{"ra": "ra", "rt": "rtw", "qr": "qr"}[name]], (key, name)


def test_blocks_name_the_columns_each_trace_is_made_of(table):
    """Post.ra = [theta; a; b], Post.rt = [zeta; lambda; sig2t], Post.qr = [beta or rho | vec(Sigp) | nu] in terms of the subject traces (0 theta, 1 zeta, 2 nu) and the
    item trace's columns [a b lambda sig2t | small part of qr]; Null's 2 (F + 1) zeros ahead of the Sigp the kernels publish at 4J + sigp_off; only CrossQr's nu is
    in device order."""
    for (model, N, J, F), t in table.items():
        key = (model, N, J, F)
        assert _blocks(t["blocks_ra"]) == [("S", N, 0, 0, False), ("I", 2 * J, N, 0, False)], key
        assert _blocks(t["blocks_rt"]) == ([("S", N, 0, 1, False), ("I", 2 * J, N, 2 * J, False)] if t["rt"] else []), key
        qr = _blocks(t["blocks_qr"])
        head = t["qr_head"] + 4 * t["rt"]
        if t["beta"] == "zero_pair":
            assert qr == [("Z", t["nbeta"], 0, 0, False), ("I", 4, t["nbeta"], 4 * J + t["sigp_off"], False)] and t["nbeta"] == 2 * (F + 1), key
        else:
            assert qr[0] == ("I", head, 0, 4 * J, False) and head == t["nq"], key
            assert qr[1:] == {"none": [], "subject": [("S", N, head, 2, False)], "cell": [("C", N * J, head, 2, True)]}[t["nu"]], key
        device_order = [b for name in ("ra", "rt", "qr", "ll") for b in _blocks(t["blocks_" + name]) if b[4]]
        assert len(device_order) == (model == pu.MODELS["crossqr"]) and all(b[0] == "C" for b in device_order), key
        # every item block lies inside the item-trace row
        assert all(0 <= b[3] and b[3] + b[1] <= t["item"] for name in ("ra", "rt", "qr") for b in _blocks(t["blocks_" + name]) if b[0] == "I"), key
