"""CPU: ``install_dropin()`` aliases only the hot-path modules and leaves the host project's ``plnn`` / ``graphnet`` packages
importable (reference call sites: plnn/relu_conv_gnnkwthreshold.py:6-7, graphnet/graph_conv.py:11).

The host project is a throw-away package tree written into tmp_path by this test (stub files of our own, NOT reference
files): ``plnn/`` with ``__init__``, ``modules`` (its own Flatten), ``sibling`` and ``relu_conv_stub`` (which does what the
reference's BaB driver does at import time), ``graphnet/`` with ``__init__``, ``graph_score``, ``graph_conv``, ``other``.
Each scenario runs in a fresh interpreter so that sys.modules starts clean.
"""
import os
import subprocess
import sys
import textwrap

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

TREE = {
    "plnn/__init__.py": "HOST_PLNN = True\n",
    "plnn/modules.py": "class Flatten:\n    origin = 'host'\n",
    "plnn/sibling.py": "VALUE = 41\n",
    "plnn/kw_score_conv.py": "def choose_node_conv(*a):\n    return 'host'\n\ndef choose_node_perturbed(*a):\n    return 'host-perturbed'\n",
    "plnn/relu_conv_stub.py": textwrap.dedent("""\
        from plnn.kw_score_conv import choose_node_conv
        from graphnet.graph_score import GraphChoice
        from plnn.modules import Flatten
        import plnn.sibling
        def where():
            return GraphChoice.__module__, Flatten.__module__, plnn.sibling.VALUE, choose_node_conv.__module__
        """),
    "graphnet/__init__.py": "HOST_GRAPHNET = True\n",
    "graphnet/graph_score.py": "class GraphChoice:\n    origin = 'host'\n",
    "graphnet/graph_conv.py": "from plnn.modules import Flatten\nclass GraphNet:\n    origin = 'host'\n",
    "graphnet/graph_score_online.py": "class GraphChoice:\n    origin = 'host-online'\n",
    "graphnet/other.py": "VALUE = 7\n",
}


def _tree(tmp_path):
    for rel, text in TREE.items():
        f = tmp_path / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(text)
    return str(tmp_path)


def _run(tmp_path, body, with_tree=True):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join(([_tree(tmp_path)] if with_tree else []) + [ROOT])
    env["PYTHONDONTWRITEBYTECODE"] = "1"
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(body)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_install_first_then_import_the_driver(tmp_path):
    out = _run(tmp_path, """
        import gnn_branching_amd
        gnn_branching_amd.install_dropin()
        import plnn.relu_conv_stub as drv                 # the host project's own module, found in ITS plnn package
        gc, fl, sib, kw = drv.where()
        assert gc == "gnn_branching_amd.graphnet.graph_score", gc
        assert fl == "gnn_branching_amd.plnn.modules", fl
        assert sib == 41 and kw == "plnn.kw_score_conv"
        import plnn, graphnet, graphnet.other
        assert plnn.HOST_PLNN and graphnet.HOST_GRAPHNET and graphnet.other.VALUE == 7     # the packages are the host's
        import graphnet.graph_conv, graphnet.graph_score, plnn.modules
        assert graphnet.graph_conv.GraphNet.__module__ == "gnn_branching_amd.graphnet.graph_conv"
        assert graphnet.graph_score is __import__("sys").modules["gnn_branching_amd.graphnet.graph_score"]
        assert plnn.modules.Flatten is gnn_branching_amd.plnn.modules.Flatten
        import graphnet.graph_score_online as on          # not aliased unless asked for
        assert on.GraphChoice.origin == "host-online"
        print("ok")
        """)
    assert out.strip().endswith("ok")


def test_install_after_the_packages_and_the_driver_were_imported(tmp_path):
    out = _run(tmp_path, """
        import plnn, graphnet, plnn.sibling
        import plnn.relu_conv_stub as drv                 # already bound the host's GraphChoice / Flatten
        assert drv.where()[0] == "graphnet.graph_score"
        import gnn_branching_amd
        gnn_branching_amd.install_dropin(online=True, babsr=True)
        gc, fl, sib, kw = drv.where()
        assert gc == "gnn_branching_amd.graphnet.graph_score", gc      # re-pointed
        assert fl == "gnn_branching_amd.plnn.modules", fl
        assert sib == 41
        assert kw == "gnn_branching_amd.plnn.kw_score_conv", kw
        from graphnet.graph_score import GraphChoice
        from graphnet.graph_conv import GraphNet
        from plnn.modules import Flatten
        assert GraphChoice.__module__.startswith("gnn_branching_amd.") and GraphNet.__module__.startswith("gnn_branching_amd.")
        import graphnet.graph_score_online as on
        assert on.GraphChoice.__module__ == "gnn_branching_amd.graphnet.graph_score_online"
        import plnn.kw_score_conv as kwm                  # the host's module keeps its other functions
        assert kwm.choose_node_perturbed() == "host-perturbed"
        assert kwm.choose_node_conv.__module__ == "gnn_branching_amd.plnn.kw_score_conv"
        assert plnn.HOST_PLNN and graphnet.HOST_GRAPHNET
        print("ok")
        """)
    assert out.strip().endswith("ok")


def test_install_without_a_host_project(tmp_path):
    """No `plnn` / `graphnet` on the path at all: stub parent packages make the aliased imports work."""
    out = _run(tmp_path, """
        import gnn_branching_amd
        gnn_branching_amd.install_dropin()
        from graphnet.graph_score import GraphChoice
        import graphnet.graph_conv
        from plnn.modules import Flatten
        assert GraphChoice.__module__ == "gnn_branching_amd.graphnet.graph_score"
        try:
            import plnn.relu_conv_gnnkwthreshold
        except ModuleNotFoundError:
            pass
        else:
            raise AssertionError("a module that exists nowhere must not resolve")
        print("ok")
        """, with_tree=False)
    assert out.strip().endswith("ok")


# A stand-in of the host project's BaB driver with the import form the drop-in has to serve: the driver
# module imports the branch-and-bound helpers, choose_node_conv and GraphChoice by name at import time; graph_score_online imports
# GraphNet from graphnet.graph_conv.  Stub files of our own, like TREE; torch is imported as a real driver does.
DRIVER_TREE = {
    "plnn/__init__.py": "",
    "plnn/branch_and_bound.py": "import bisect\nimport torch\n\ndef pick_out(*a):\n    pass\n\ndef add_domain(*a):\n    pass\n\n"
                                "def prune_domains(*a):\n    pass\n",
    "plnn/kw_score_conv.py": "def choose_node_conv(*a):\n    return 'host'\n",
    "plnn/modules.py": "class Flatten:\n    origin = 'host'\n",
    "plnn/relu_conv_gnnkwthreshold.py": textwrap.dedent("""\
        import torch
        from plnn.branch_and_bound import pick_out, add_domain, prune_domains
        from torch import nn
        from plnn.kw_score_conv import choose_node_conv
        from graphnet.graph_score import GraphChoice
        def relu_gnn(*a):
            return GraphChoice
        """),
    "graphnet/__init__.py": "",
    "graphnet/graph_conv.py": "import torch\nclass GraphNet:\n    origin = 'host'\n",
    "graphnet/graph_score.py": "class GraphChoice:\n    origin = 'host'\n",
    "graphnet/graph_score_online.py": "import torch\nfrom graphnet.graph_conv import GraphNet\nclass GraphChoice:\n    origin = 'host-online'\n",
}


def test_reference_driver_imports_after_install(tmp_path):
    """The host project's BaB driver module (stand-in with the reference driver's import form) imports with the drop-in installed and
    binds this package's GraphChoice -- the call order INTEGRATION.md section A documents; the host's other graphnet modules stay its own."""
    host = tmp_path / "host"
    for rel, text in DRIVER_TREE.items():
        f = host / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(text)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(host), ROOT]), PYTHONDONTWRITEBYTECODE="1")
    body = textwrap.dedent(f"""
        import gnn_branching_amd
        gnn_branching_amd.install_dropin()
        from plnn.relu_conv_gnnkwthreshold import relu_gnn
        import plnn.branch_and_bound
        import plnn.relu_conv_gnnkwthreshold as m
        assert m.GraphChoice.__module__ == "gnn_branching_amd.graphnet.graph_score"
        assert relu_gnn() is m.GraphChoice
        import graphnet.graph_score_online as on
        assert on.__file__.startswith({str(host) + os.sep!r})
        print("ok")
        """)
    r = subprocess.run([sys.executable, "-c", body], env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
