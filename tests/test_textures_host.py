"""The host side of the texture path (csrc/png_decode.cpp, csrc/collada.cpp, csrc/capi.cpp), no device:

- PNG decode: files written here with zlib and struct -- colour types 0, 2, 3, 4, 6; each scanline filter 0-4 on every row and a mix of all
  five; sizes 1x1, 1x7, 7x1, 5x3; IDAT in one chunk and split (inside the zlib header too); palettes with and without tRNS; ancillary chunks
  around IDAT -- decode to source bytes / 256 (texture.rs:35-49: `to_rgb8()` drops alpha and expands grey and palette), PIL-written files to
  PIL's convert("RGB"); all of them through bin/dae2scene on a minimal COLLADA document and back through scene_io;
- documents with several images: a material's texture id is the image's position in library_images (colladaloader.rs), whatever order the
  effects use them in, and two materials may share one image;
- malformed PNG and scene files are refused with a RuntimeError that names the cause, in a fresh child process each, which must end with
  status 0: no exception leaves a C entry point, and a header is not believed (nothing of the declared size is allocated) before the file's
  data bears it out.  A refused file never reaches the device, so this is host work on any machine."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "raytracer-rs_amd", "bin", "dae2scene")
F = np.float32
SIG = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
SIZES = [(1, 1), (1, 7), (7, 1), (5, 3)]                 # (width, height)
FILTERS = [0, 1, 2, 3, 4, "mix"]


# ---- a PNG writer (PNG specification, second edition: 5.3 chunk layout, 9.2 filter types) ---------------------------------------------------
def chunk(kind, data=b""):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def ihdr(w, h, ctype, depth=8, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def filtered(pix, filters):
    """the scanlines of pix uint8[h, w, ch], row y under filter type filters[y], each behind its filter byte"""
    h, w, ch = pix.shape
    rows = [[int(x) for x in pix[y].reshape(-1)] for y in range(h)]
    out = bytearray()
    for y in range(h):
        cur, up = rows[y], rows[y - 1] if y else [0] * (w * ch)
        out.append(filters[y])
        for i, x in enumerate(cur):
            a = cur[i - ch] if i >= ch else 0
            b = up[i]
            c = up[i - ch] if i >= ch else 0
            pred = [0, a, b, (a + b) // 2, paeth(a, b, c)][filters[y]]
            out.append((x - pred) & 0xFF)
    return bytes(out)


def split_at(data, cuts):
    cuts = [0] + sorted(c for c in cuts if 0 <= c <= len(data)) + [len(data)]
    return [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def png(pix, ctype, filters=0, cuts=(), plte=None, trns=None, before=(), after=()):
    h, w, ch = pix.shape
    assert ch == CHANNELS[ctype]
    rows = [(y + w) % 5 for y in range(h)] if filters == "mix" else [filters] * h
    stream = zlib.compress(filtered(pix, rows), 6)
    out = SIG + ihdr(w, h, ctype)
    if plte is not None:
        out += chunk(b"PLTE", bytes(plte))
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    for c in before:
        out += c
    for part in split_at(stream, cuts):
        out += chunk(b"IDAT", part)
    for c in after:
        out += c
    return out + chunk(b"IEND")


def pixels(rng, w, h, ctype, ncolours=256):
    return rng.integers(0, ncolours if ctype == 3 else 256, (h, w, CHANNELS[ctype]), dtype=np.uint8)


def as_rgb(pix, ctype, plte=None):
    """image::DynamicImage::to_rgb8: grey -> (g, g, g), alpha dropped, palette looked up"""
    if ctype in (0, 4):
        return np.repeat(pix[:, :, :1], 3, axis=2)
    if ctype == 3:
        return np.asarray(plte, np.uint8).reshape(-1, 3)[pix[:, :, 0]]
    return pix[:, :, :3]


def texels(rgb8):
    return rgb8.astype(F) / F(256.0)                     # texture.rs:42-44


# ---- a COLLADA document around a list of images ---------------------------------------------------------------------------------------------
def collada(images, effects):
    """images: [(id, file name)] in library_images order; effects: per material, an image id (a textured effect) or an (r, g, b).  Material i
    owns one triangle, geometry i, in node order: scene material i."""
    fx, mats, geoms, nodes = [], [], [], []
    for i, e in enumerate(effects):
        if isinstance(e, str):
            params = ('<newparam sid="s%d-surface"><surface type="2D"><init_from>%s</init_from></surface></newparam>'
                      '<newparam sid="s%d-sampler"><sampler2D><source>s%d-surface</source></sampler2D></newparam>' % (i, e, i, i))
            diffuse = '<texture texture="s%d-sampler" texcoord="map"/>' % i
        else:
            params, diffuse = "", '<color sid="diffuse">%g %g %g 1</color>' % tuple(e)
        fx.append('<effect id="m%d-effect"><profile_COMMON>%s<technique sid="common"><lambert><emission><color sid="emission">0 0 0 1</color></emission>'
                  '<diffuse>%s</diffuse><index_of_refraction><float sid="ior">1.45</float></index_of_refraction></lambert></technique></profile_COMMON></effect>'
                  % (i, params, diffuse))
        mats.append('<material id="m%d-material"><instance_effect url="#m%d-effect"/></material>' % (i, i))
        geoms.append('<geometry id="g%d-mesh"><mesh><source id="g%d-mesh-positions"><float_array id="g%d-mesh-positions-array" count="9">%d 0 0 %d 0 0 %d 1 0'
                     '</float_array></source><triangles material="m%d-material" count="1"><p>0 0 0 1 0 1 2 0 2</p></triangles></mesh></geometry>'
                     % (i, i, i, 2 * i, 2 * i + 1, 2 * i, i))
        nodes.append('<node id="n%d"><matrix sid="transform">1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 1</matrix><instance_geometry url="#g%d-mesh"/></node>' % (i, i))
    imgs = "".join('<image id="%s" name="%s"><init_from>%s</init_from></image>' % (a, a, b) for a, b in images)
    return """<?xml version="1.0" encoding="utf-8"?>
<COLLADA xmlns="http://www.collada.org/2005/11/COLLADASchema" version="1.4.1">
  <asset><up_axis>Z_UP</up_axis></asset>
  <library_cameras><camera id="Cam-camera"><optics><technique_common><perspective>
     <xfov sid="xfov">39.59775</xfov><aspect_ratio>1.777778</aspect_ratio></perspective></technique_common></optics></camera></library_cameras>
  <library_lights><light id="L-light"><technique_common><point><color sid="color">10 10 10</color></point></technique_common></light></library_lights>
  <library_effects>%s</library_effects>
  <library_images>%s</library_images>
  <library_materials>%s</library_materials>
  <library_geometries>%s</library_geometries>
  <library_visual_scenes><visual_scene id="Scene">%s
     <node id="L"><matrix sid="transform">1 0 0 1 0 1 0 2 0 0 1 3 0 0 0 1</matrix><instance_light url="#L-light"/></node>
     <node id="C"><matrix sid="transform">1 0 0 0 0 1 0 0 0 0 1 5 0 0 0 1</matrix><instance_camera url="#Cam-camera"/></node>
  </visual_scene></library_visual_scenes>
  <scene><instance_visual_scene url="#Scene"/></scene>
</COLLADA>
""" % ("".join(fx), imgs, "".join(mats), "".join(geoms), "".join(nodes))


def decode_all(scene_io, tmp_path, files):
    """files: {file name: bytes}.  Writes them beside a document with one textured material per file, runs dae2scene, reads the container back:
    {file name: float32[h, w, 3]}"""
    names = sorted(files)
    for n in names:
        (tmp_path / n).write_bytes(files[n])
    ids = ["img%d" % i for i in range(len(names))]
    (tmp_path / "doc.dae").write_text(collada(list(zip(ids, names)), ids))
    subprocess.run([TOOL, str(tmp_path / "doc.dae"), str(tmp_path / "doc.scene")], check=True, capture_output=True, text=True)
    sc = scene_io.load_scene_file(str(tmp_path / "doc.scene"))
    assert list(sc["mat_kind"]) == [1] * len(names) and list(sc["mat_tex"]) == list(range(len(names)))
    assert len(sc["textures"]) == len(names)
    return dict(zip(names, sc["textures"]))


def same(got, want):
    return got.shape == want.shape and got.dtype == np.float32 and np.array_equal(got.view(np.uint32), np.ascontiguousarray(want, F).view(np.uint32))


ANCILLARY_BEFORE = (chunk(b"gAMA", struct.pack(">I", 45455)), chunk(b"pHYs", struct.pack(">IIB", 2835, 2835, 1)), chunk(b"tEXt", b"Comment\0before the data"))
ANCILLARY_AFTER = (chunk(b"tEXt", b"Comment\0after the data"), chunk(b"tIME", struct.pack(">HBBBBB", 2024, 2, 29, 12, 0, 0)))


# ---- 1. PNG decode ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", [0, 2, 3, 4, 6])
def test_png_decode_every_filter_size_and_chunking(pkg, scene_io, tmp_path, ctype):
    from PIL import Image
    rng = np.random.default_rng(100 + ctype)
    plte = rng.integers(0, 256, 3 * 200, dtype=np.uint8) if ctype == 3 else None          # 200 entries: indices stay below it
    files, want = {}, {}

    def add(name, pix, **kw):
        files[name] = png(pix, ctype, plte=plte, **kw)
        want[name] = as_rgb(pix, ctype, plte)

    for w, h in SIZES:
        for f in FILTERS:
            add("f%s_%dx%d.png" % (f, w, h), pixels(rng, w, h, ctype, 200), filters=f)
    pix = pixels(rng, 5, 3, ctype, 200)
    n = len(zlib.compress(filtered(pix, [(y + 5) % 5 for y in range(3)]), 6))
    assert n > 8
    for label, cuts in [("zlib_header", [1]), ("three", [1, 5, n - 2]), ("with_empty", [4, 4, 9]), ("every_byte", list(range(1, n)))]:
        add("split_%s.png" % label, pix, filters="mix", cuts=cuts)
    add("ancillary.png", pix, filters=4, cuts=[7], before=ANCILLARY_BEFORE, after=ANCILLARY_AFTER)
    if ctype == 3:
        files["trns.png"] = png(pix, 3, filters=3, plte=plte, trns=rng.integers(0, 256, 200, dtype=np.uint8))
        want["trns.png"] = as_rgb(pix, 3, plte)
        files["trns_short.png"] = png(pix, 3, filters=1, plte=plte, trns=[0])
        want["trns_short.png"] = as_rgb(pix, 3, plte)
    got = decode_all(scene_io, tmp_path, files)
    for name in sorted(files):
        # the writer above is not trusted either: PIL reads the same file to the same pixels
        pil = np.asarray(Image.open(str(tmp_path / name)).convert("RGB"))
        assert np.array_equal(pil, want[name]), name
        assert same(got[name], texels(want[name])), name
    assert sorted((y + 1) % 5 for y in range(7)) == [0, 1, 1, 2, 2, 3, 4]                   # filters="mix" gives the 1x7 file all five types


@pytest.mark.parametrize("mode", ["L", "LA", "RGB", "RGBA", "P", "P+transparency"])
def test_png_decode_of_files_written_by_pil(pkg, scene_io, tmp_path, mode):
    from PIL import Image
    rng = np.random.default_rng(7)
    files = {}
    for w, h in SIZES + [(33, 9)]:
        base = mode.split("+")[0]
        a = rng.integers(0, 256, (h, w, {"L": 1, "LA": 2, "RGB": 3, "RGBA": 4, "P": 1}[base]), dtype=np.uint8)
        im = Image.frombytes(base, (w, h), a.tobytes())
        kw = {}
        if base == "P":
            im.putpalette([int(x) for x in rng.integers(0, 256, 768)])
            if "+" in mode:
                kw["transparency"] = bytes(int(x) for x in rng.integers(0, 256, 256))
        name = "pil_%dx%d.png" % (w, h)
        im.save(str(tmp_path / name), **kw)
        files[name] = (tmp_path / name).read_bytes()
        assert files[name][24] == 8 and files[name][28] == 0, "the input must be an 8-bit, non-interlaced file"
    got = decode_all(scene_io, tmp_path, files)
    for name in files:
        want = np.asarray(Image.open(str(tmp_path / name)).convert("RGB"))
        assert same(got[name], texels(want)), name


# ---- 2. documents with several images ---------------------------------------------------------------------------------------------------------
def three_images(tmp_path):
    rng = np.random.default_rng(11)
    plte = rng.integers(0, 256, 3 * 256, dtype=np.uint8)
    spec = {"grey.png": (0, 7, 2), "rgba.png": (6, 3, 5), "pal.png": (3, 4, 4)}          # colour type, width, height
    rgb = {}
    for name, (ctype, w, h) in spec.items():
        pix = pixels(rng, w, h, ctype)
        (tmp_path / name).write_bytes(png(pix, ctype, filters="mix", plte=plte if ctype == 3 else None))
        rgb[name] = texels(as_rgb(pix, ctype, plte))
    return rgb


def test_texture_ids_follow_library_images_not_the_effects(pkg, scene_io, tmp_path):
    rgb = three_images(tmp_path)
    images = [("img-pal", "pal.png"), ("img-grey", "grey.png"), ("img-rgba", "rgba.png")]     # document order: texture ids 0, 1, 2
    effects = ["img-rgba", (0.25, 0.5, 0.75), "img-grey", "img-rgba", (0.125, 0.0, 1.0), "img-pal"]
    (tmp_path / "multi.dae").write_text(collada(images, effects))
    log = subprocess.run([TOOL, str(tmp_path / "multi.dae"), str(tmp_path / "multi.scene")], check=True, capture_output=True, text=True).stdout
    assert "geometries 6 lights 1 cameras 1 textures 3" in log
    sc = scene_io.load_scene_file(str(tmp_path / "multi.scene"))
    assert list(sc["tri_geom"]) == [0, 1, 2, 3, 4, 5]
    assert list(sc["mat_kind"]) == [1, 0, 1, 1, 0, 1]
    assert [int(t) for t, k in zip(sc["mat_tex"], sc["mat_kind"]) if k] == [2, 1, 2, 0]
    assert np.array_equal(sc["mat_rgb"][1], np.array([0.25, 0.5, 0.75], F)) and np.array_equal(sc["mat_rgb"][4], np.array([0.125, 0.0, 1.0], F))
    assert [t.shape for t in sc["textures"]] == [(4, 4, 3), (2, 7, 3), (5, 3, 3)]
    for t, name in zip(sc["textures"], ["pal.png", "grey.png", "rgba.png"]):
        assert same(t, rgb[name]), name


def test_an_effect_naming_a_missing_image_is_an_error(pkg, tmp_path):
    three_images(tmp_path)
    (tmp_path / "missing.dae").write_text(collada([("img-pal", "pal.png")], ["img-pal", "img-nowhere"]))
    r = subprocess.run([TOOL, str(tmp_path / "missing.dae"), str(tmp_path / "missing.scene")], capture_output=True, text=True)
    assert r.returncode == 1 and "MaterialsConversion error; can't find texture name" in r.stderr
    with pytest.raises(RuntimeError, match="MaterialsConversion error; can't find texture name"):
        pkg.create_raytracer_from_file(str(tmp_path / "missing.dae"), pkg.DEFAULT_TRIANGLES_PER_LEAF, 8, 8)


# ---- 3. malformed files are refused, not fatal -----------------------------------------------------------------------------------------------
CHILD = """
import resource, sys
sys.path.insert(0, %r)
import __graft_entry__ as ge
pkg = ge.load_package()
create = pkg.create_raytracer_from_scene_file if sys.argv[1].endswith(".scene") else pkg.create_raytracer_from_file
try:
    create(sys.argv[1], pkg.DEFAULT_TRIANGLES_PER_LEAF, 8, 8)
    print("CREATED")
except RuntimeError as e:
    print("RuntimeError: %%s" %% e)
print("maxrss_kb %%d" %% resource.getrusage(resource.RUSAGE_SELF).ru_maxrss)
""" % ROOT


def refused(path):
    """create from `path` in a fresh process; the process must end with status 0 having printed the RuntimeError's text, which is returned,
    with the peak resident size of the child in KiB"""
    r = subprocess.run([sys.executable, "-c", CHILD, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, "the child ended with status %d\n%s\n%s" % (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("RuntimeError: ") and lines[1].startswith("maxrss_kb "), r.stdout
    return lines[0][len("RuntimeError: "):], int(lines[1].split()[1])


def grey_idat(w, h):
    return chunk(b"IDAT", zlib.compress(b"".join(b"\0" + bytes([40 + y] * w) for y in range(h))))


def raw_png(w, h, ctype, body, depth=8, interlace=0):
    return SIG + ihdr(w, h, ctype, depth, interlace) + body + chunk(b"IEND")


def malformed_pngs():
    one_rgba = chunk(b"IDAT", zlib.compress(b"\0\1\2\3\4"))
    pal = chunk(b"IDAT", zlib.compress(b"\0\0\1\2" + b"\0\2\1\0"))                  # 3 x 2, indices 0-2
    whole = raw_png(4, 3, 0, grey_idat(4, 3))
    return {
        "ihdr_ffffffff": (raw_png(0xFFFFFFFF, 0xFFFFFFFF, 0, grey_idat(4, 3)), "IDAT too short for the declared image size"),
        "size_wraps": (raw_png(0x40000000, 0x80000000, 6, one_rgba), "IDAT too short for the declared image size"),
        "40000_squared": (raw_png(40000, 40000, 6, one_rgba), "IDAT too short for the declared image size"),
        "one_row_short": (raw_png(4, 4, 0, grey_idat(4, 3)), "corrupt deflate stream"),
        "16_bit": (raw_png(4, 3, 0, chunk(b"IDAT", zlib.compress((b"\0" + b"\0\1" * 4) * 3)), depth=16), "Unsupported PNG (only 8-bit non-interlaced images are handled)"),
        "interlaced": (raw_png(4, 3, 0, grey_idat(4, 3), interlace=1), "Unsupported PNG (only 8-bit non-interlaced images are handled)"),
        "no_idat": (raw_png(4, 3, 0, b""), "missing IDAT"),
        "palette_without_plte": (raw_png(3, 2, 3, pal), "missing PLTE"),
        "short_plte": (raw_png(3, 2, 3, chunk(b"PLTE", bytes(range(6))) + pal), "palette index out of range"),
        "filter_byte_5": (raw_png(4, 3, 0, chunk(b"IDAT", zlib.compress(b"\0" + b"\7" * 4 + b"\5" + b"\7" * 4 + b"\0" + b"\7" * 4))), "bad filter type"),
        "truncated_chunk": (whole[:len(whole) - 12 - 9], "truncated chunk"),
        "bad_signature": (b"\x89PNG\r\n\x1a\r" + whole[8:], "Invalid PNG signature"),
        "garbage_deflate": (raw_png(4, 3, 0, chunk(b"IDAT", b"\x78\x9c" + bytes(range(40)))), "corrupt deflate stream"),
    }


PNG_CASES = malformed_pngs()


@pytest.mark.parametrize("case", sorted(PNG_CASES))
def test_a_malformed_png_is_refused_not_fatal(pkg, tmp_path, case):
    data, message = PNG_CASES[case]
    (tmp_path / "t.png").write_bytes(data)
    (tmp_path / "doc.dae").write_text(collada([("img", "t.png")], ["img"]))
    text, maxrss_kb = refused(tmp_path / "doc.dae")
    assert message in text, text
    assert maxrss_kb < 1 << 20, "the child grew to %d KiB: the declared size was allocated" % maxrss_kb     # the lies are 6.4 GB and up
    r = subprocess.run([TOOL, str(tmp_path / "doc.dae"), str(tmp_path / "doc.scene")], capture_output=True, text=True)
    assert r.returncode == 1 and message in r.stderr                                         # the converter: an error, not a signal


def scene_bytes(counts=None, textures=((3, 2, 1), (2, 2, 0)), texels_written=None):
    """a small valid container (the layout of scene_io.load_scene_file); counts overrides the five header counts; texels_written: the number of
    texels that follow each texture's header, where that is not the width * height it declares"""
    ntri, nmat, nlight, ncam = 2, 2, 1, 1
    body = np.arange(ntri * 9, dtype=F).tobytes() + np.array([0, 1], np.uint32).tobytes()
    body += struct.pack("<I3fI", 1, 0.0, 0.0, 0.0, 1) + struct.pack("<I3fI", 0, 0.5, 0.25, 1.0, 0)
    body += struct.pack("<6f", -3.0, 2.0, 1.0, 1.0, 1.0, 1.0)
    body += np.eye(4, dtype=F).tobytes() + struct.pack("<f", 40.0)
    sections = {"triangles": 28 + 10, "tri_geom": 28 + ntri * 36 + 2, "materials": 28 + ntri * 40 + 22, "lights": 28 + ntri * 40 + nmat * 20 + 5,
                "cameras": 28 + ntri * 40 + nmat * 20 + 24 + 30}
    for i, (w, h, as_bytes) in enumerate(textures):
        sections["texture_%d_header" % i] = 28 + len(body) + 6
        body += struct.pack("<3I", w, h, as_bytes)
        sections["texture_%d_texels" % i] = 28 + len(body) + 4
        n = 3 * (w * h if texels_written is None else texels_written)
        body += bytes(range(n)) if as_bytes else (np.arange(n, dtype=F) / F(7.0)).tobytes()
    head = b"M355SCN1" + struct.pack("<5I", *(counts or (ntri, nmat, nlight, len(textures), ncam)))
    return head + body, sections


def malformed_scenes():
    whole, sections = scene_bytes()
    cases = {"header_cut": (whole[:20], "truncated scene file")}
    for field, what in [(0, "the triangles"), (1, "the materials"), (3, "the textures")]:
        counts = [0, 0, 0, 0, 0]
        counts[field] = 0xFFFFFFFF
        cases["count_%d_ffffffff" % field] = (b"M355SCN1" + struct.pack("<5I", *counts), "truncated scene file: " + what)
    cases["every_count_ffffffff"] = (b"M355SCN1" + struct.pack("<5I", *([0xFFFFFFFF] * 5)), "truncated scene file: the triangles")
    cases["texture_ffff_squared_floats"] = (scene_bytes(textures=((0xFFFF, 0xFFFF, 0),), texels_written=4)[0], "truncated scene file: the texels of a texture")
    cases["texture_ffffffff_squared_bytes"] = (scene_bytes(textures=((0xFFFFFFFF, 0xFFFFFFFF, 1),), texels_written=4)[0], "truncated scene file: the texels of a texture")
    for name, cut in sections.items():
        cases["cut_in_" + name] = (whole[:cut], "truncated scene file")
    cases["last_byte_missing"] = (whole[:-1], "truncated scene file")
    cases["bad_magic"] = (b"M355SCN2" + whole[8:], "not a scene file")
    return cases


SCENE_CASES = malformed_scenes()


@pytest.mark.parametrize("case", sorted(SCENE_CASES))
def test_a_malformed_scene_file_is_refused_not_fatal(pkg, scene_io, tmp_path, case):
    data, message = SCENE_CASES[case]
    (tmp_path / "t.scene").write_bytes(data)
    text, maxrss_kb = refused(tmp_path / "t.scene")
    assert message in text, text
    assert maxrss_kb < 1 << 20, "the child grew to %d KiB: a count of the file was believed" % maxrss_kb


def test_the_scene_file_the_cases_are_cut_from_is_valid(pkg, scene_io, tmp_path):
    """the uncut container reads back as written, bytes and floats, so each refusal above is owed to its cut alone"""
    whole, _ = scene_bytes()
    (tmp_path / "t.scene").write_bytes(whole)
    sc = scene_io.load_scene_file(str(tmp_path / "t.scene"))
    assert sc["tri_verts"].shape == (2, 9) and list(sc["mat_kind"]) == [1, 0] and list(sc["mat_tex"]) == [1, 0]
    assert same(sc["textures"][0], (np.arange(18, dtype=np.uint8).astype(F) / F(256.0)).reshape(2, 3, 3))
    assert same(sc["textures"][1], (np.arange(12, dtype=F) / F(7.0)).reshape(2, 2, 3))
    text, _ = refused(tmp_path / "t.scene") if not _has_device() else ("no HIP device", 0)
    assert "no HIP device" in text                                                            # the file itself loads: only the device is missing


def _has_device():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:       # noqa: BLE001
        return False
