"""``client survey run --where COLUMN OP VALUE / --predicate`` end to end: one
CN and two file-loader DPs as real server processes on localhost (the setup of
tests/test_sql_cli.py), "mean of c0 where c2 >= 2" and "where c2 = 0 or c1 =
1" over their record files; comparison operators together with --predicate
are refused before the configuration is even read."""
import os
import socket
import subprocess
import time

from test_cli import PY, ROOT, _port, _run

FILES = {1: [(10, 0, 1), (20, 1, 2), (30, 0, 0), (50, 1, 3)],
         2: [(40, 0, 2), (70, 0, 1), (90, 1, 0), (11, 5, 3)]}  # (c0, c1, c2)
ENV = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")


def test_operators_with_a_predicate_are_refused_before_anything_is_read():
    for args in (["--where", "c2>=2", "--predicate", "v0 >= v1"],
                 ["--where", "c2=1", "--where", "c1<3", "--predicate", "v0 == v1 || v2 < v3"]):
        r = subprocess.run(PY + ["drynx_amd.cli.client", "survey", "run"] + args, input="", capture_output=True,
                           text=True, cwd=ROOT, timeout=300, env=ENV)
        # no configuration on stdin: reading it would have failed on the missing network instead
        assert r.returncode != 0 and "together with --predicate" in r.stderr and "Network" not in r.stderr


def test_filtered_mean_over_record_files(tmp_path):
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
                                 stderr=subprocess.PIPE, text=True, cwd=ROOT, env=ENV)
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
        sv = _run(["drynx_amd.cli.client", "survey", "new", "predicate-survey"], net)
        sv = _run(["drynx_amd.cli.client", "survey", "set-operation", "mean"], sv)
        rows = [r for rs in FILES.values() for r in rs]
        # an operator in --where: the CLI writes the conjunction formula itself
        out = _run(["drynx_amd.cli.client", "survey", "run", "--where", "c2>=2"], sv)
        want = [r[0] for r in rows if r[2] >= 2]
        assert len(want) == 4 and abs(float(out.strip()) - sum(want) / len(want)) < 1e-9
        # a formula of the caller's over equality terms, grouped
        out = _run(["drynx_amd.cli.client", "survey", "run", "--group-by", "c1", "--cardinalities", "2",
                    "--where", "c2=0", "--where", "c0 == 20", "--predicate", "v0 == v1 || v2 == v3"], sv)
        lines = out.strip().splitlines()
        assert [ln.split(":")[0] for ln in lines] == ["[0]", "[1]"]
        for g, ln in enumerate(lines):
            want = [r[0] for r in rows if (r[2] == 0 or r[0] == 20) and r[1] == g]
            assert want and abs(float(ln.split(":")[1]) - sum(want) / len(want)) < 1e-9
        # a malformed formula is refused by the query rules before the survey is sent
        r = subprocess.run(PY + ["drynx_amd.cli.client", "survey", "run", "--where", "c2=1", "--predicate", "v0 = v1"],
                           input=sv, capture_output=True, text=True, cwd=ROOT, timeout=300, env=ENV)
        assert r.returncode != 0 and "not valid" in r.stderr
    finally:
        from drynx_amd.services.server import RemoteNode

        RemoteNode(addrs[0]).shutdown()
        for p in procs:
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                p.kill()
