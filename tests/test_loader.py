"""COLLADA ingest (raytracer-rs_amd/csrc/collada.cpp): against an independent numpy/ElementTree
restatement of colladaloader.rs:137-273 + collada_types.rs:76-90 on the reference's bundled files
(stored xz-compressed under tests/golden/collada/), and its error behaviour on inline documents."""
import lzma
import os
import shutil
import subprocess
import xml.etree.ElementTree as ET

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLLADA = os.path.join(ROOT, "tests", "golden", "collada")         # the reference's data files: *.dae.xz + the ico3 texture
NS = "{http://www.collada.org/2005/11/COLLADASchema}"
f32 = np.float32


def matmul_ref(s, r):
    """vecmath.rs:237-313: left-to-right f32 sums"""
    o = np.zeros(16, f32)
    for i in range(4):
        for j in range(4):
            o[4 * i + j] = ((s[4 * i] * r[j] + s[4 * i + 1] * r[4 + j]) + s[4 * i + 2] * r[8 + j]) + s[4 * i + 3] * r[12 + j]
    return o


def to_vecmath(c):
    c = np.asarray(c, f32)
    row_major = c.reshape(4, 4).T.reshape(-1).copy()
    swap = np.array([1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 1], f32)
    refl = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1], f32)
    return matmul_ref(matmul_ref(refl, row_major), swap)


def xform(m, v):
    v = np.asarray(v, f32)
    return np.array([((v[0] * m[j] + v[1] * m[4 + j]) + v[2] * m[8 + j]) + f32(1.0) * m[12 + j] for j in range(3)], f32)


def numpy_loader(path):
    root = ET.parse(path).getroot()
    geoms = {}
    for g in root.find(NS + "library_geometries"):
        gid = g.get("id")
        mesh = g.find(NS + "mesh")
        pos = None
        for src in mesh.findall(NS + "source"):
            if src.get("id") == gid + "-positions":
                pos = np.array(src.find(NS + "float_array").text.split(), f32).reshape(-1, 3)
        tri = mesh.find(NS + "triangles")
        idx = np.array(tri.find(NS + "p").text.split(), np.int64)[::3]
        geoms[gid] = (pos, idx, tri.get("material"))
    effects = {}
    for e in root.find(NS + "library_effects"):
        col = e.find(".//" + NS + "diffuse/" + NS + "color")
        effects[e.get("id")] = None if col is None else np.array(col.text.split(), f32)[:3]
    materials = {m.get("id"): m.find(NS + "instance_effect").get("url")[1:] for m in root.find(NS + "library_materials")}
    verts, geom_ids, mats, lights, cams = [], [], [], [], []
    for node in root.find(NS + "library_visual_scenes").iter(NS + "node"):
        m = to_vecmath(np.array(node.find(NS + "matrix").text.split(), f32))
        if node.find(NS + "instance_light") is not None:
            lid = node.find(NS + "instance_light").get("url")[1:]
            for l in root.find(NS + "library_lights"):
                if l.get("id") == lid:
                    color = np.array(l.find(".//" + NS + "color").text.split(), f32)
                    lights.append(np.concatenate([xform(m, [0, 0, 0]), color]))
        elif node.find(NS + "instance_geometry") is not None:
            pos, idx, mat = geoms[node.find(NS + "instance_geometry").get("url")[1:]]
            verts.append(np.stack([xform(m, pos[i]) for i in idx]))
            geom_ids.append(np.full(len(idx) // 3, len(mats), np.uint32))
            mats.append(effects[materials[mat]])
        elif node.find(NS + "instance_camera") is not None:
            cams.append(m)
    return np.concatenate(verts).reshape(-1, 9), np.concatenate(geom_ids), mats, np.stack(lights), cams


@pytest.mark.parametrize("name", ["4boxes", "ico2", "thai2", "ico3_tex"])
def test_cpp_loader_matches_independent_numpy_loader(pkg, scene_io, name, tmp_path):
    tool = os.path.join(ROOT, "raytracer-rs_amd", "bin", "dae2scene")
    dae = tmp_path / (name + ".dae")
    with lzma.open(os.path.join(COLLADA, name + ".dae.xz")) as f:
        dae.write_bytes(f.read())
    shutil.copy(os.path.join(COLLADA, "blender_cycles_ico3.png"), tmp_path)    # textures are found next to the document
    out = tmp_path / (name + ".scene")
    log = subprocess.check_output([tool, str(dae), str(out)], text=True)
    sc = scene_io.load_scene_file(str(out))
    assert "number of triangles: %d" % sc["tri_geom"].size in log          # colladaloader.rs:265
    committed = open(os.path.join(ROOT, "tests", "golden", "scenes", name + ".scene"), "rb").read()
    assert open(out, "rb").read() == committed                             # fixtures are reproducible
    verts, geom, mats, lights, cams = numpy_loader(str(dae))
    assert np.array_equal(sc["tri_verts"].view(np.uint32), verts.view(np.uint32))     # bit-exact world-space vertices
    assert np.array_equal(sc["tri_geom"], geom)
    assert np.array_equal(sc["lights"].view(np.uint32), lights.view(np.uint32))
    assert np.array_equal(sc["camera_matrix"].view(np.uint32), cams[0].view(np.uint32))
    for i, m in enumerate(mats):
        if m is None:
            assert sc["mat_kind"][i] == 1 and sc["mat_tex"][i] == 0        # Diffuse::TextureId
        else:
            assert sc["mat_kind"][i] == 0 and np.array_equal(sc["mat_rgb"][i], m)
    if name == "ico3_tex":
        from PIL import Image
        img = np.asarray(Image.open(os.path.join(COLLADA, "blender_cycles_ico3.png")).convert("RGB"), np.float32) / f32(256.0)
        assert np.array_equal(sc["textures"][0], img)                      # texture.rs:35-49


DOC = """<?xml version="1.0" encoding="utf-8"?>
<COLLADA xmlns="http://www.collada.org/2005/11/COLLADASchema" version="1.4.1">
  <asset><up_axis>Z_UP</up_axis></asset>
  <library_cameras><camera id="Cam-camera"><optics><technique_common><perspective>
     <xfov sid="xfov">39.59775</xfov><aspect_ratio>1.777778</aspect_ratio></perspective></technique_common></optics></camera></library_cameras>
  <library_lights><light id="L-light"><technique_common><point><color sid="color">10 10 10</color></point></technique_common></light></library_lights>
  <library_effects><effect id="M-effect"><profile_COMMON><technique sid="common"><lambert>
     <emission><color sid="emission">0 0 0 1</color></emission><diffuse><color sid="diffuse">0.8 0.1 0.2 1</color></diffuse>
     <index_of_refraction><float sid="ior">1.45</float></index_of_refraction></lambert></technique></profile_COMMON></effect></library_effects>
  <library_images/>
  <library_materials><material id="M-material"><instance_effect url="#M-effect"/></material></library_materials>
  <library_geometries><geometry id="T-mesh"><mesh>
     <source id="T-mesh-positions"><float_array id="T-mesh-positions-array" count="9">0 0 0 1 0 0 0 1 0</float_array></source>
     <triangles material="M-material" count="1"><p>0 0 0 1 0 1 2 0 2</p></triangles></mesh></geometry></library_geometries>
  <library_visual_scenes><visual_scene id="Scene">
     <node id="T"><matrix sid="transform">1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 1</matrix><instance_geometry url="#T-mesh"/></node>
     <node id="L"><matrix sid="transform">1 0 0 1 0 1 0 2 0 0 1 3 0 0 0 1</matrix><instance_light url="#L-light"/></node>
     <node id="C"><matrix sid="transform">1 0 0 0 0 1 0 0 0 0 1 5 0 0 0 1</matrix><instance_camera url="#Cam-camera"/></node>
  </visual_scene></library_visual_scenes>
  <scene><instance_visual_scene url="#Scene"/></scene>
</COLLADA>
"""


def create_error(pkg, doc):
    with pytest.raises(RuntimeError) as e:
        pkg.create_raytracer(doc, pkg.DEFAULT_TRIANGLES_PER_LEAF, 16, 16)
    return str(e.value)


def test_loader_error_strings(pkg):
    """Result<RayTracer, String> errors of create_raytracer (lib.rs:15-20): ColladaError Display prefixes."""
    import torch
    ok = create_error(pkg, DOC) if not torch.cuda.is_available() else None
    if ok is not None:
        assert "no HIP device" in ok                                         # the document itself loads
    assert "LibraryImagesParsing error" in create_error(pkg, DOC.replace("<library_images/>", ""))
    assert "XmlDefinition error" in create_error(pkg, DOC.split("\n", 1)[1])
    assert create_error(pkg, DOC.replace("COLLADA", "COLLADB")) == "Not a collada doc"
    assert "RemainingData error" in create_error(pkg, DOC + "trailing")
    assert "VisualSceneConversion error; unsupported node type" in create_error(pkg, DOC.replace('<instance_camera url="#Cam-camera"/>', ""))
    assert "ElementError error" in create_error(pkg, DOC.replace("<xfov sid=\"xfov\">39.59775</xfov>", ""))
    assert "GeometryConversion error" in create_error(pkg, DOC.replace("0 0 0 1 0 1 2 0 2", "0 0 0 1 0 1 2 0"))
    assert "scene has no camera" in create_error(pkg, DOC.replace('<library_cameras><camera id="Cam-camera">', '<library_cameras><camera id="Other">'))
    with pytest.raises(RuntimeError, match="No such file"):
        pkg.create_raytracer_from_file("/nonexistent/x.dae", 70, 16, 16)
