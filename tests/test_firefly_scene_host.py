"""scenes.firefly_spheres() on the CPU: reflective_spheres() plus one small, very bright emitter as the LAST object, which no primary ray of the 64 x 36
frame sees (the oracle's own rays and intersections) — so its light arrives only through bounces that happen to hit it: fireflies by construction.
Python only: no benchmark configuration names it."""
import numpy as np

import oracle_lib
from raymond_amd import scenes
from raymond_amd.scene import Settings


def test_it_is_reflective_spheres_plus_one_emitter():
    base, scene = scenes.reflective_spheres(), scenes.firefly_spheres()
    assert len(scene.objects) == len(base.objects) + 1
    centre, radius, emission = scenes.FIREFLY_EMITTER
    assert emission == (1500.0, 1500.0, 1500.0) and radius == 0.05  # 1000 times the ceiling's (1.5, 1.5, 1.5)
    assert all(name != "firefly_spheres" for name, *_ in scenes.CONFIGS.values())


def test_no_primary_ray_hits_the_emitter_and_bounces_do():
    W, H, spp = 64, 36, 16
    scene = scenes.firefly_spheres()
    emitter = len(scene.objects) - 1
    cam = scenes.camera(W, H)
    st = Settings(cam, sample_count=spp, bounce_limit=5, seed=scenes.SEED)
    yy, xx = np.mgrid[0:H, 0:W]
    xy = np.repeat(np.stack([xx.ravel(), yy.ravel()], axis=1), spp, axis=0).astype(np.uint32)
    samples = np.tile(np.arange(spp, dtype=np.uint32), W * H)
    rays, ok = oracle_lib.sample_primary_rays(cam, st.seed, False, xy, samples)
    assert ok.all()
    o = oracle_lib.OracleScene(scene)
    obj, _, _ = o.scene_intersect(rays)
    assert (obj != emitter).all() and (obj >= 0).all()  # every first hit is a wall or one of the two spheres
    first_base, _, _ = oracle_lib.OracleScene(scenes.reflective_spheres()).scene_intersect(rays)
    assert np.array_equal(obj, first_base)
    # ... and a bounce can reach it: from points the camera sees on the floor, the ceiling and the red sphere's top the emitter is the first hit towards it
    centre = np.array(scenes.FIREFLY_EMITTER[0])
    origins = np.array([(0.0, -0.999, 2.0), (1.8, -0.999, 1.0), (1.0, 1.999, 3.0), (-1.0, 0.001, 3.5)])
    towards = centre - origins
    towards /= np.linalg.norm(towards, axis=1, keepdims=True)
    seen, _, _ = o.scene_intersect(np.concatenate([origins, towards], axis=1))
    assert (seen == emitter).all()
