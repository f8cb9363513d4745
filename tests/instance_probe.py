"""Child process of tests/test_instance_table_cpu.py and tests/test_gpu_instances.py: the rows of
tests/instance_table.py that need A/B switches, under the environment it was started with (the libraries read their
switches once per process).   python tests/instance_probe.py dry|gpu
dry: every such row's launcher in dry-run on poisoned host buffers; gpu: every such row launched and checked as
tests/test_gpu_instances.py checks a row. One line `ok <row name>` per row that passed; exit status 0 if all did.
python tests/instance_probe.py pairs <nx> <ny> <nz>   (tests/test_gpu_switches.py): one line per launch, `<call> <mode>
<kernel>`, of what the LINEAR plain pair and the LINEAR and GS_NEWTON_B prolongation pairs launch on that level under
this environment, asked of the launch record in dry-run."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "..", "gpu-solve_amd"), os.path.join(HERE, "..", "oracle")):
    sys.path.insert(0, p)
import instance_table as IT  # noqa: E402

what = sys.argv[1]
if what == "pairs":
    shape = tuple(int(a) for a in sys.argv[2:5])
    for call, mode in (("pair", 0), ("prolong", 0), ("prolong", 3)):
        r = IT.Row("k_tb2y", "?", call, shape, mode)
        IT.dry_run(r, True)
        rc, names = IT.launch(r, IT.HostSide())
        IT.dry_run(r, False)
        assert rc == 0, (r, rc)
        for n in names:
            print(call, mode, n)
    sys.exit(0)
rows = [r for r in IT.rows() if r.env]
assert all(os.environ.get(k) == v for r in rows for k, v in r.env.items()), "started without the rows' switches"
if what == "dry":
    for r in rows:
        IT.dry_run(r, True)
        R = IT.HostSide()
        rc, names = IT.launch(r, R)
        IT.dry_run(r, False)
        assert rc == 0 and names == r.launches and R.untouched(), (r, rc, names)
        print("ok", r.name)
else:
    import test_gpu_instances as G
    for r in rows:
        G.check_row(r)
        print("ok", r.name)
