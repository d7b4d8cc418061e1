"""Are the images of this build the images of another build, to the last byte?

  python tools/render_cmp.py --parent-tree DIR [--envs N]   DIR: a checkout of the other commit with its library built (its
                                                            own package loads it)
  python tools/render_cmp.py [--envs N]                     the other build is safe_adaptation_gym_amd/libsag_rold.so, loaded
                                                            by this tree's package (same ABI and exports only)

N envs (512; a small batch for the host build of the device sources) of three robot / task pairs after 30 steps.  Per pair: the
first-person image; two human-view sizes with overlays in colour, depth and segmentation, whole batch (the first 64 rows) and
a listed subset; and the masked device forms (render_rows_device, render_aux_device) into a sentinel-filled buffer.  Each
build renders in a process of its own; exit status 1 when an array differs.  With SAG_HOSTEMU=1 in the environment each tree
loads its own unsanitized host build of the device sources (tests/hostemu/build.py --cc clang --no-san) instead."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = {'rgb': 3, 'depth': 4, 'segmentation': 8}   # bytes per pixel


def one(tree, path, n):
  sys.path.insert(0, tree)
  import bench
  out = {}
  ids = [n - 1, 0, n // 2, 0, n // 3]   # any order, a duplicate
  mask = ((np.arange(n) % 3 == 0) * (1 + np.arange(n) % 255)).astype(np.uint8)   # every third env, bytes other than 1
  for robot, task in (('doggo', 'haul_box'), ('point', 'push_box'), ('car', 'press_buttons')):
    r = bench.DeviceRun(task, n, 0, 0, robot=robot)
    r.burn_in(30)
    c = r.ctx
    out[f'{robot} vision rgb'] = c.render_rgb()
    for cam, (w, h) in ((1, (96, 72)), (2, (130, 50))):
      for output in OUTPUTS:
        kw = dict(camera=cam, width=w, height=h, overlays=True, output=output)
        out[f'{robot} cam {cam} {w}x{h} {output}'] = c.render(**kw)[:64]
        out[f'{robot} cam {cam} {w}x{h} {output} listed'] = c.render(envs=ids, **kw)
    d_mask = c.dev_alloc(n)
    c.dev_upload(d_mask, mask)
    for output, size in OUTPUTS.items():
      fill = np.full((n, 64 * 64 * size), 0xA5, np.uint8)
      d_out = c.dev_alloc(fill.nbytes)
      c.dev_upload(d_out, fill)
      if output == 'rgb':
        c.render_rows_device(d_mask, d_out)
      else:
        c.render_aux_device(output, d_out, d_mask)
      c.wait()
      out[f'{robot} vision {output} masked'] = got = c.dev_download(d_out, fill.shape, np.uint8)
      assert (got[mask == 0] == 0xA5).all() and not (got[mask != 0] == 0xA5).all(1).any(), f'{robot} {output}: not the rows of the mask'
      c.dev_free(d_out)
    c.dev_free(d_mask)
  np.savez(path, **{k.replace(' ', '_'): v for k, v in out.items()})


def main():
  a = sys.argv[1:]
  parent = os.path.abspath(a[a.index('--parent-tree') + 1]) if '--parent-tree' in a else None
  n = a[a.index('--envs') + 1] if '--envs' in a else '512'
  with tempfile.TemporaryDirectory() as tmp:
    for name, tree, lib in (('new', ROOT, None), ('old', parent or ROOT, None if parent else os.path.join(ROOT, 'safe_adaptation_gym_amd', 'libsag_rold.so'))):
      env = dict(os.environ)
      env.pop('SAG_LIB', None)
      if env.get('SAG_HOSTEMU'):
        lib = os.path.join(tree, 'tests', 'hostemu', '_build', 'libsag_hostemu_clang_nosan.so')
      if lib:
        env['SAG_LIB'] = lib
      subprocess.check_call([sys.executable, os.path.abspath(__file__), 'one', tree, os.path.join(tmp, name + '.npz'), n], env=env, cwd=tree)
    x, y = np.load(os.path.join(tmp, 'new.npz')), np.load(os.path.join(tmp, 'old.npz'))
    same = True
    for k in x.files:
      eq = np.array_equal(x[k], y[k])
      same = same and eq
      print(k, x[k].shape, 'identical' if eq else f'DIFFER in {(x[k] != y[k]).sum()} bytes')
  sys.exit(0 if same else 1)


if __name__ == '__main__':
  if len(sys.argv) > 1 and sys.argv[1] == 'one':
    one(sys.argv[2], sys.argv[3], int(sys.argv[4]))
  else:
    main()
