"""GPU: kernel time of one context after burn-in and its busy env count, as one JSON line (tools/quick4m.sh runs it per switch setting).
  python tools/busy_e_sweep.py one <task> <robot> <envs>"""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) != 5 or sys.argv[1] != 'one':
  sys.exit(__doc__)
sys.path.insert(0, ROOT)
import bench
task, robot, n = sys.argv[2], sys.argv[3], int(sys.argv[4])
run = bench.DeviceRun(task, n, 0, 0, robot=robot)
run.burn_in(200); run.timing(True); run.run(40); run.wait()
print(json.dumps({'ms': run.kernel_time_ms()[0], 'busy': run.ctx.busy_count()}))
