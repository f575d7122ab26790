"""sim.py / test.py --srgb IMG --unprocess against the oracle's files, the *.raw route on them and the develop export."""
import os
import struct
import zlib

import numpy as np
import pytest

from conftest import GOLDEN
from calib_cases import load_test_py
from helpers import same

import develop_oracle as DO
import unprocess_oracle as UO

pytestmark = pytest.mark.gpu
XYZ2CAM = [1.0234, -0.2969, -0.2266, -0.5625, 1.6328, -0.0469, -0.0703, 0.2188, 0.6406]
CAMERA = ["--colormatrix"] + [str(v) for v in XYZ2CAM] + ["--red-gain", "2.1", "--blue-gain", "1.6", "--curve", "srgb"]
SENSOR = ["--cfa", "grbg", "--black", "64", "--white", "1023"]


def test_sim_from_an_image_to_a_developed_png(tmp_path, capsys):
    import sim
    from sesrq import develop, image, unprocess
    from sesrq.store import STORE
    img = np.random.default_rng(5).integers(0, 256, (40, 52, 3), dtype=np.uint8)
    img[4:12] |= 0xE0
    src, rawp, gtp, png = (str(tmp_path / n) for n in ("in.npy", "f_40_52.raw", "gt.png", "dev.png"))
    np.save(src, img)
    base = ["--mflag", "3", "--params", os.path.join(GOLDEN, "nrdm_3_nat.params.npz")]
    STORE.clear()
    y = sim.main(base + ["--srgb", src, "--image", "--unprocess", "--no-highlight", "--save-raw", rawp, "--save-gt", gtp, "--develop",
                         "--save-png", png] + CAMERA + SENSOR)
    assert "nrdm_small mean psnr is:" in capsys.readouterr().out
    p = unprocess.from_colormatrix(XYZ2CAM, 2.1, 1.6, curve="srgb", highlight=False)
    k = UO.codes(img[None], p.curve, p.rgb2cam, p.inv_gains, False, "rgb", 1023 - 64)
    want = UO.outputs(k, "grbg", 64, 1023)
    same("--save-raw", np.fromfile(rawp, "<u2").reshape(1, 40, 52), want["raw"])
    blob = open(gtp, "rb").read()                                       # --save-gt: a 16-bit RGB PNG of black + k_c
    assert blob[12:16] == b"IHDR" and struct.unpack(">IIBB", blob[16:26]) == (52, 40, 16, 2)
    rows = np.frombuffer(zlib.decompress(blob[blob.index(b"IDAT") + 4:-16]), np.uint8).reshape(40, 1 + 6 * 52)
    same("--save-gt", rows[:, 1:].copy().view(">u2").astype(np.uint16).reshape(40, 52, 3), (64 + k[0]).astype(np.uint16).transpose(1, 2, 0))
    STORE.clear()
    y2 = sim.main(base + ["--input", rawp] + SENSOR)                    # the *.raw route on the saved frame
    same("output", y, y2)
    dp = develop.from_colormatrix(XYZ2CAM, 2.1, 1.6, curve="srgb")
    same("--develop --save-png", image.load_image(png), DO.export(y.cpu().numpy(), dp.gains, dp.ccm, dp.curve)[0])


def test_test_py_calibrates_from_images(tmp_path, capsys):
    from sesrq import unprocess
    from sesrq.store import STORE
    mod = load_test_py()
    p = unprocess.from_colormatrix(XYZ2CAM, 2.1, 1.6, curve="srgb")
    files = [[str(tmp_path / f"{n}{i}{ext}") for i in range(2)] for n, ext in (("i", ".npy"), ("r", "_40_52.raw"), ("g", ".npy"))]
    for src, rawp, gtp in zip(*files):
        img = np.random.default_rng(len(src)).integers(0, 256, (40, 52, 3), dtype=np.uint8)
        k = UO.codes(img[None], p.curve, p.rgb2cam, p.inv_gains, True, "rgb", 1023 - 64)
        np.save(src, img), np.save(gtp, (64 + k).astype(np.uint16))
        UO.outputs(k, "grbg", 64, 1023)["raw"].astype("<u2").tofile(rawp)
    base = ["--mflag", "3", "--params", os.path.join(GOLDEN, "nrdm_3.params.npz")] + SENSOR
    res = []
    for args in (["--srgb", *files[0], "--image", "--unprocess"] + CAMERA, ["--input", *files[1], "--gt", *files[2]]):
        STORE.clear()
        domains = mod.main(base + args)
        res.append(([list(v) for v in domains], [l for l in capsys.readouterr().out.split("\n") if "psnr" in l]))
    assert res[0] == res[1] and len(res[0][1]) == 1
