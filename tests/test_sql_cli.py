"""``client survey run --group-by / --cardinalities / --where`` end to end:
one CN and two file-loader DPs as real server processes on localhost, "mean of
c0 where c2 = 1, by c1" over their record files (the setup of
tests/test_cli.py::test_role_filters_and_file_loader)."""
import os
import socket
import subprocess
import time

from test_cli import PY, ROOT, _port, _run

FILES = {1: [(10, 0, 1), (20, 1, 1), (30, 0, 0), (50, 1, 1)],
         2: [(40, 0, 1), (70, 0, 1), (90, 1, 0), (11, 5, 1)]}  # (c0, c1, c2); c1 = 5 is outside the two groups


def test_grouped_mean_over_record_files(tmp_path):
    addrs = [f"127.0.0.1:{_port()}" for _ in range(3)]
    procs = []
    try:
        cfgs = []
        for i, a in enumerate(addrs):
            cfg = _run(["drynx_amd.cli.server", "new", a])
            if i == 0:
                cfg = _run(["drynx_amd.cli.server", "computing-node", "new"], cfg)
            else:
                f = tmp_path / f"dp{i}.csv"
                f.write_text("".join(",".join(str(v) for v in r) + "\n" for r in FILES[i]))
                cfg = _run(["drynx_amd.cli.server", "data-provider", "new", "file-loader", str(f)], cfg)
            cfgs.append(cfg)
        pubs = [[ln.split('"')[1] for ln in cfg.splitlines() if ln.startswith("Public")][0] for cfg in cfgs]
        group = _run(["drynx_amd.cli.client", "network", "new"])
        for a, pub in zip(addrs, pubs):
            group = _run(["drynx_amd.cli.client", "network", "add-node", a, pub], group)
        (tmp_path / "group.toml").write_text(group)
        for i, cfg in enumerate(cfgs):
            p = subprocess.Popen(PY + ["drynx_amd.cli.server", "run", "--workdir", str(tmp_path / f"n{i}"),
                                       "--device", "cpu", "--group", str(tmp_path / "group.toml")],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, text=True, cwd=ROOT,
                                 env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
            p.stdin.write(cfg)
            p.stdin.close()
            procs.append(p)
        for a in addrs:
            host, port = a.split(":")
            for _ in range(300):
                try:
                    socket.create_connection((host, int(port)), timeout=1).close()
                    break
                except OSError:
                    time.sleep(0.2)
        net = _run(["drynx_amd.cli.client", "network", "set-client", addrs[0]], group)
        sv = _run(["drynx_amd.cli.client", "survey", "new", "sql-survey"], net)
        sv = _run(["drynx_amd.cli.client", "survey", "set-operation", "mean"], sv)
        out = _run(["drynx_amd.cli.client", "survey", "run", "--group-by", "c1", "--cardinalities", "2",
                    "--where", "c2=1"], sv)
        rows = [r for rs in FILES.values() for r in rs if r[2] == 1]
        want = {g: [r[0] for r in rows if r[1] == g] for g in range(2)}
        lines = out.strip().splitlines()
        assert [ln.split(":")[0] for ln in lines] == ["[0]", "[1]"]
        for g, ln in enumerate(lines):
            assert abs(float(ln.split(":")[1]) - sum(want[g]) / len(want[g])) < 1e-9
        # a malformed --where never reaches the servers
        r = subprocess.run(PY + ["drynx_amd.cli.client", "survey", "run", "--where", "c2"], input=sv,
                           capture_output=True, text=True, cwd=ROOT, timeout=300,
                           env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
        assert r.returncode != 0 and "COLUMN=VALUE" in r.stderr
    finally:
        from drynx_amd.services.server import RemoteNode

        RemoteNode(addrs[0]).shutdown()
        for p in procs:
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                p.kill()
