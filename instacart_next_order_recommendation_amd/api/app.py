"""FastAPI app: /health /ready /metrics, POST /recommend, POST /admin/corpus.

Follows the reference's src/api/main.py:51-166 (lifespan, request-id middleware, probes,
metrics endpoint), src/api/routes/recommend.py:84-199 (context resolution, response assembly,
Prometheus observations), src/api/routes/corpus.py:47-106 (re-index on upload) and
src/api/auth.py:39-71 (X-API-Key / Bearer).  Differences, all deliberate:
  * requests go to a Backend (batcher.py): a LocalBackend micro-batches them in front of this process's recommender
    instead of a blocking call on the event loop, a RemoteBackend (remote.py) forwards them to the GPU-owner processes;
    the routes do not know which one they talk to;
  * eval_queries.json is cached (the reference re-parses it on every user_id request, :40-63,:115);
  * no slowapi rate limiter (its 100/min default would throttle any throughput measurement);
  * feedback endpoints are out of scope.
Env: MODEL_DIR, CORPUS_PATH, API_KEY, INFERENCE_DEVICE, MAX_CORPUS_UPLOAD_PRODUCTS,
     BATCH_MAX_SIZE (256), BATCH_MAX_WAIT_MS (2).
     ICREC_GPU_WORKER_SOCKET: this process is an HTTP front-end of the multi-process server (serve.py): it loads
     the corpus JSON only and forwards every request to the GPU-owner process(es) (worker.py; a comma-separated list of
     sockets = several GPU owners on one GPU, requests round-robin: serve.py --gpu-workers N hands every front-end all
     of them).
"""
from __future__ import annotations

import asyncio
import json
import logging
import os
import tempfile
import time
from contextlib import asynccontextmanager
from pathlib import Path
from typing import AsyncIterator, Optional
from uuid import uuid4

from fastapi import Depends, FastAPI, HTTPException, Request, Response, status
from prometheus_client import CONTENT_TYPE_LATEST, generate_latest
from starlette.datastructures import State

from ..recommender import MonitoredRecommender
from . import DEFAULT_CORPUS_PATH, DEFAULT_MODEL_DIR
from .batcher import Backend, LocalBackend
from .metrics import (API_REGISTRY, MODEL_LOADED, RECOMMENDATION_BATCH_SIZE, RECOMMENDATION_ENCODE_SECONDS,
                      RECOMMENDATION_LATENCY_SECONDS, RECOMMENDATION_REQUESTS_TOTAL)
from .remote import RemoteBackend, WorkerUnavailable
from .schemas import (CorpusUploadRequest, CorpusUploadResponse, HealthResponse, InferenceStatistics,
                      RecommendationItem, RecommendationRequest, RecommendationResponse)
from .worker import settle_heap

logger = logging.getLogger(__name__)

EVAL_QUERIES_FILENAME = "eval_queries.json"  # src/constants.py:55
DEFAULT_MAX_CORPUS_UPLOAD_PRODUCTS = 100_000  # src/constants.py:83


async def _load_backend(app: FastAPI) -> Backend:
    """Build this process's backend from the environment and install it (lifespan, or the first request without one)."""
    corpus_path = Path(os.getenv("CORPUS_PATH") or DEFAULT_CORPUS_PATH)
    socks = os.getenv("ICREC_GPU_WORKER_SOCKET")
    if socks:
        backend = RemoteBackend([p for p in socks.split(",") if p], corpus_path)
    else:
        model_dir = Path(os.getenv("MODEL_DIR") or DEFAULT_MODEL_DIR)
        logger.info("Loading recommender model_dir=%s corpus=%s", model_dir, corpus_path)
        # in a worker thread (model upload + catalog encode): the event loop keeps answering probes meanwhile
        backend = await asyncio.to_thread(
            LocalBackend, lambda cp: MonitoredRecommender(model_dir=model_dir, corpus_path=cp), corpus_path,
            max_batch=int(os.getenv("BATCH_MAX_SIZE", "256")), max_wait_ms=float(os.getenv("BATCH_MAX_WAIT_MS", "2")))
    await backend.start()
    app.state.backend = backend  # from here on /ready says so
    MODEL_LOADED.set(1)
    return backend


@asynccontextmanager
async def lifespan(app: FastAPI) -> AsyncIterator[None]:
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    await _load_backend(app)
    settle_heap()
    try:
        yield
    finally:
        MODEL_LOADED.set(0)
        if app.state.backend is not None:
            await app.state.backend.stop()


class _AppState(State):
    """`app.state.recommender` reads through to the backend's: one holder, nothing to keep in step at a swap."""

    @property
    def recommender(self):
        return self.backend and self.backend.recommender


app = FastAPI(title="Instacart Next-Order Recommendation API (MI355X)", lifespan=lifespan)
app.state = _AppState({"backend": None})


class RequestIdMiddleware:
    """X-Request-ID propagation + request log line (reference: src/api/main.py request_logging_middleware) as a
    plain ASGI middleware: Starlette's BaseHTTPMiddleware costs a task group and two memory streams per
    request, which at micro-batched rates is a visible share of the per-request budget."""

    def __init__(self, inner):
        self.inner = inner

    async def __call__(self, scope, receive, send):
        if scope["type"] != "http":
            await self.inner(scope, receive, send)
            return
        start = time.time()
        req_id = None
        for k, v in scope.get("headers") or ():
            if k == b"x-request-id":
                req_id = v.decode("latin-1")
                break
        req_id = req_id or str(uuid4())
        scope.setdefault("state", {})["request_id"] = req_id
        status_code = 0

        async def send_with_id(message):
            nonlocal status_code
            if message["type"] == "http.response.start":
                status_code = message["status"]
                message.setdefault("headers", [])
                message["headers"] = list(message["headers"]) + [(b"x-request-id", req_id.encode("latin-1"))]
            await send(message)

        await self.inner(scope, receive, send_with_id)
        if logger.isEnabledFor(logging.DEBUG):
            logger.debug("request path=%s method=%s status=%d request_id=%s latency_ms=%d", scope.get("path"),
                         scope.get("method"), status_code, req_id, int((time.time() - start) * 1000))


app.add_middleware(RequestIdMiddleware)


async def verify_api_key(request: Request) -> None:
    """When API_KEY is set, require it as X-API-Key or `Authorization: Bearer` (src/api/auth.py)."""
    expected = os.getenv("API_KEY")
    if not expected:
        return
    got = request.headers.get("X-API-Key")
    if not got:
        auth = request.headers.get("Authorization", "")
        if auth.lower().startswith("bearer "):
            got = auth[7:].strip()
    if got != expected:
        raise HTTPException(status_code=status.HTTP_401_UNAUTHORIZED, detail="Invalid or missing API key")


_lazy_lock: Optional[asyncio.Lock] = None


async def get_backend(request: Request) -> Backend:  # async: a sync dependency costs a thread-pool hop per request
    """The app's backend; loaded ON DEMAND when the lifespan did not run or failed to install one - the reference's
    fallback (src/api/routes/recommend.py:76-80: a MonitoredRecommender constructed inside the dependency).  Two
    differences: concurrent first requests wait for ONE load instead of each starting their own, and a load that fails
    answers 503 with the reason (the reference lets the exception become a 500)."""
    backend = request.app.state.backend
    if backend is not None:
        return backend
    global _lazy_lock
    if _lazy_lock is None:
        _lazy_lock = asyncio.Lock()
    async with _lazy_lock:
        if request.app.state.backend is not None:
            return request.app.state.backend
        logger.warning("Recommender not preloaded; loading on-demand")
        try:
            return await _load_backend(request.app)
        except Exception as exc:  # noqa: BLE001
            logger.exception("on-demand load failed")
            raise HTTPException(status_code=status.HTTP_503_SERVICE_UNAVAILABLE,
                                detail=f"recommender not loaded: {exc.__class__.__name__}: {exc}") from exc


def _eval_queries(app: FastAPI, corpus_path: Path) -> dict[str, str]:
    """eval_queries.json next to the corpus, cached by (path, mtime)."""
    path = Path(corpus_path).parent / EVAL_QUERIES_FILENAME
    try:
        mtime = path.stat().st_mtime
    except OSError:
        return {}
    cache = getattr(app.state, "eval_queries_cache", None)
    if cache and cache[0] == (str(path), mtime):
        return cache[1]
    try:
        data = json.loads(path.read_text())
        data = {str(k): str(v) for k, v in data.items()} if isinstance(data, dict) else {}
    except (OSError, ValueError):
        logger.exception("Failed to load %s", path)
        data = {}
    app.state.eval_queries_cache = ((str(path), mtime), data)
    return data


@app.get("/health", response_model=HealthResponse)
async def health() -> HealthResponse:
    return HealthResponse(status="ok")


@app.get("/ready", response_model=HealthResponse)
async def ready(request: Request) -> HealthResponse:
    backend = request.app.state.backend
    # a front-end of the multi-process server is connected only while its sockets to the GPU-owner processes are up
    ok = backend is not None and backend.connected
    return HealthResponse(status="ready" if ok else "not_ready")


@app.get("/metrics")
async def metrics() -> Response:
    return Response(content=generate_latest(API_REGISTRY), media_type=CONTENT_TYPE_LATEST)


@app.post("/recommend", response_model=RecommendationResponse, status_code=status.HTTP_200_OK)
async def recommend_endpoint(payload: RecommendationRequest, request: Request,
                             backend: Backend = Depends(get_backend),
                             _: None = Depends(verify_api_key)) -> RecommendationResponse:
    start_time = time.perf_counter()
    try:
        context = payload.user_context
        if context is None and payload.user_id is not None:
            context = _eval_queries(request.app, backend.corpus_path).get(str(payload.user_id))
        if payload.query is not None and payload.query.strip():
            retrieval_query = f"{payload.query} {context}" if context else payload.query
        else:
            retrieval_query = context
        if not retrieval_query:
            raise HTTPException(
                status_code=status.HTTP_400_BAD_REQUEST,
                detail="Either query (optional) must be provided, or user_context must be provided / user_id must be resolvable.")

        request_id = str(uuid4())
        exclude_ids = set(payload.exclude_product_ids or [])
        user_id_str = str(payload.user_id) if payload.user_id is not None else None
        stats = None
        texts = backend.pid_to_text  # before the await: of the catalog that answers, whatever is swapped in meanwhile
        t_submit = time.time()
        try:
            results, tm = await backend.submit(retrieval_query, payload.top_k, exclude_ids, user_id_str)
        except WorkerUnavailable as exc:  # front-end mode: the GPU-owner process is gone
            raise HTTPException(status_code=status.HTTP_503_SERVICE_UNAVAILABLE, detail=str(exc)) from exc
        if tm is not None:  # answered out of a batch
            RECOMMENDATION_BATCH_SIZE.observe(tm.batch_size)
            if backend.stats:
                n = len(results)
                stats = InferenceStatistics(
                    total_latency_ms=(time.time() - t_submit) * 1000, query_embedding_time_ms=tm.encode_ms,
                    similarity_compute_time_ms=tm.search_ms, num_recommendations=n,
                    top_score=results[0][1] if results else 0.0,
                    avg_score=sum(s for _, s in results) / n if n else 0.0, timestamp=time.time())
                RECOMMENDATION_ENCODE_SECONDS.observe(tm.encode_ms / 1000.0)
        items = [RecommendationItem(product_id=pid, score=score, product_text=texts.get(pid)) for pid, score in results]
        RECOMMENDATION_LATENCY_SECONDS.observe(time.perf_counter() - start_time)
        RECOMMENDATION_REQUESTS_TOTAL.labels(status="success").inc()
        return RecommendationResponse(request_id=request_id, recommendations=items, stats=stats,
                                      purchase_history_used=context)
    except Exception:
        RECOMMENDATION_REQUESTS_TOTAL.labels(status="error").inc()
        raise


@app.post("/admin/corpus", response_model=CorpusUploadResponse)
async def corpus_upload_endpoint(payload: CorpusUploadRequest, request: Request,
                                 _: None = Depends(verify_api_key),
                                 backend: Backend = Depends(get_backend)) -> CorpusUploadResponse:
    """Replace the catalog: write it to a JSON file and have the backend re-index from it (a NEW recommender, full GPU
    re-encode, swapped in; reference: routes/corpus.py:47-106)."""
    limit = int(os.getenv("MAX_CORPUS_UPLOAD_PRODUCTS", str(DEFAULT_MAX_CORPUS_UPLOAD_PRODUCTS)))
    if len(payload.corpus) > limit:
        raise HTTPException(status_code=status.HTTP_413_REQUEST_ENTITY_TOO_LARGE,
                            detail=f"corpus has {len(payload.corpus)} products; limit is {limit}")
    corpus_path = Path(tempfile.mkdtemp(prefix="icrec_corpus_")) / "eval_corpus.json"
    corpus_path.write_text(json.dumps(payload.corpus))
    try:
        await backend.reindex(corpus_path)
    except Exception as exc:  # noqa: BLE001
        raise HTTPException(status_code=status.HTTP_500_INTERNAL_SERVER_ERROR,
                            detail=f"Failed to load corpus: {exc}") from exc
    return CorpusUploadResponse(status="ok", n_products=len(payload.corpus))
