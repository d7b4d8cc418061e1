"""Are the colour images of this build the images of another build, to the last byte?

  python tools/render_cmp.py --parent-tree DIR     DIR: a checkout of the other commit with its library built (its own
                                                   package loads it)
  python tools/render_cmp.py                       the other build is safe_adaptation_gym_amd/libsag_rold.so, loaded by
                                                   this tree's package (same ABI and exports only)

512 envs of three robot / task pairs after 30 steps: the first-person image and two human-view sizes with overlays.  Each
build renders in a process of its own; exit status 1 when an image differs."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(tree, path):
  sys.path.insert(0, tree)
  import bench
  out = []
  for robot, task in (('doggo', 'haul_box'), ('point', 'push_box'), ('car', 'press_buttons')):
    r = bench.DeviceRun(task, 512, 0, 0, robot=robot)
    r.burn_in(30)
    out.append(r.ctx.render_rgb())
    for cam, (w, h) in ((1, (96, 72)), (2, (130, 50))):
      out.append(r.ctx.render(camera=cam, width=w, height=h, overlays=True)[:64])
  np.savez(path, *out)


def main():
  a = sys.argv[1:]
  parent = os.path.abspath(a[a.index('--parent-tree') + 1]) if '--parent-tree' in a else None
  with tempfile.TemporaryDirectory() as tmp:
    for name, tree, lib in (('new', ROOT, None), ('old', parent or ROOT, None if parent else os.path.join(ROOT, 'safe_adaptation_gym_amd', 'libsag_rold.so'))):
      env = dict(os.environ)
      env.pop('SAG_LIB', None)
      if lib:
        env['SAG_LIB'] = lib
      subprocess.check_call([sys.executable, os.path.abspath(__file__), 'one', tree, os.path.join(tmp, name + '.npz')], env=env, cwd=tree)
    x, y = np.load(os.path.join(tmp, 'new.npz')), np.load(os.path.join(tmp, 'old.npz'))
    same = True
    for k in x.files:
      eq = np.array_equal(x[k], y[k])
      same = same and eq
      print(k, x[k].shape, 'identical' if eq else f'DIFFER in {(x[k] != y[k]).sum()} bytes')
  sys.exit(0 if same else 1)


if __name__ == '__main__':
  if len(sys.argv) > 1 and sys.argv[1] == 'one':
    one(sys.argv[2], sys.argv[3])
  else:
    main()
